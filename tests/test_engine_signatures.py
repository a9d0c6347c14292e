"""engine.SIGNATURES, engine.RESTYPES, the three struct mirrors and the constants against include/glass.h: the ctypes side of the drop-in
boundary is written by hand, the header is what the library is compiled from.  A wrong width here is memory corruption in the library, not
a Python error, so drift has to fail as text.  No GPU, no built library.  The header reader is tests/abi_header.py."""
import ctypes as C

import pytest

import abi_header as H
from clip_glass_amd import engine

# what glass.h is known to use: the scalars, [const] T* (and T name[n] as a parameter), strings both ways, the opaque engine handle, void**,
# the three structs by pointer, the noise planes, and char as the element of a name buffer
VOCAB = H.vocabulary({"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double},
                     {"glass_engine*": C.c_void_p, "glass_engine**": C.POINTER(C.c_void_p), "void**": C.POINTER(C.c_void_p),
                      "const glass_config*": C.POINTER(engine.GlassConfig), "const glass_noise*": C.POINTER(engine.GlassNoise),
                      "glass_prof_row*": C.POINTER(engine.ProfRow), "const char*": C.c_char_p, "char*": C.c_char_p, "char": C.c_char,
                      "const float* const*": C.POINTER(C.POINTER(C.c_float))})
SRC = H.header("glass.h")
PROTOS, RETURNS = H.prototypes(SRC, VOCAB)
DEFINES = H.defines(SRC)


def test_signature_table_lists_exactly_the_declared_functions():
    assert len(PROTOS) >= 72
    assert sorted(engine.SIGNATURES) == sorted(PROTOS)


def test_every_signature_matches_its_prototype():
    wrong = {name: (engine.SIGNATURES.get(name), args) for name, args in PROTOS.items() if engine.SIGNATURES.get(name) != args}
    assert not wrong, "engine.SIGNATURES disagrees with include/glass.h (table, header): %s" % wrong


def test_every_restype_matches_its_prototype():
    wrong = {name: (engine.RESTYPES.get(name, C.c_int), ret) for name, ret in RETURNS.items() if engine.RESTYPES.get(name, C.c_int) != ret}
    assert not wrong, "engine.RESTYPES disagrees with include/glass.h (table, header): %s" % wrong
    assert set(engine.RESTYPES) <= set(PROTOS) and C.c_int not in engine.RESTYPES.values()      # only the exceptions are listed
    assert sorted(engine.RESTYPES) == ["glass_engine_destroy", "glass_last_error", "glass_version"]


@pytest.mark.parametrize("mirror,struct,least", [(engine.GlassConfig, "glass_config", 38), (engine.GlassNoise, "glass_noise", 3),
                                                 (engine.ProfRow, "glass_prof_row", 5)])
def test_struct_mirror_matches_the_struct(mirror, struct, least):
    declared = H.struct_fields(SRC, struct, VOCAB)
    assert len(declared) >= least
    for i, (mine, theirs) in enumerate(zip(mirror._fields_, declared)):
        assert tuple(mine) == theirs, "%s field %d: engine.%s has %r, include/glass.h declares %r" % (struct, i, mirror.__name__, mine, theirs)
    assert [f[0] for f in mirror._fields_] == [f[0] for f in declared]                           # neither side has fields left over


def test_constants_match_the_defines():
    assert engine.MAX_BLOCKS == DEFINES["GLASS_MAX_BLOCKS"] and engine.MAX_BG_LAYERS == DEFINES["GLASS_MAX_BG_LAYERS"]
    assert engine.GEN_STYLEGAN2 == DEFINES["GLASS_GEN_STYLEGAN2"] and engine.GEN_BIGGAN_DEEP == DEFINES["GLASS_GEN_BIGGAN_DEEP"]
    assert engine.LATENT_SPACES == {"z": DEFINES["GLASS_LATENT_Z"], "w": DEFINES["GLASS_LATENT_W"], "w+": DEFINES["GLASS_LATENT_WPLUS"],
                                    "sub": DEFINES["GLASS_LATENT_SUB"]}
    assert engine.SEARCH_ALGORITHMS == {"ga": DEFINES["GLASS_SEARCH_GA"], "nsga2": DEFINES["GLASS_SEARCH_NSGA2"],
                                        "cmaes": DEFINES["GLASS_SEARCH_CMAES"]}
    assert DEFINES["GLASS_OK"] == 0 and DEFINES["GLASS_ERR_ARG"] == -1                          # (negative values are read too)


# The seven forms the glass_ops.h test refuses, and a struct passed by value.  A vocabulary belongs to a header: glass.h declares `const
# char*` parameters (VOCAB reads them as strings), so that one form is refused under a vocabulary without it, as glass_ops.h's is.
NO_CONST_STRING = {k: t for k, t in VOCAB.items() if k != "const char*"}


@pytest.mark.parametrize("text,vocab", [("int32_t", VOCAB), ("const float** x", VOCAB), ("size_t n", VOCAB), ("const char* s", NO_CONST_STRING),
                                        ("glass_conv_desc* d", VOCAB), ("float (*f)", VOCAB), ("int32_t x, y", VOCAB),
                                        ("glass_config cfg", VOCAB)])
def test_parser_refuses_what_it_does_not_know(text, vocab):
    with pytest.raises(AssertionError):
        H.parameter(text, vocab)


# a function pointer, an array bound that is neither a number nor a #define, two pointer declarators on one line
@pytest.mark.parametrize("decl", ["int (*on_row)(int32_t row)", "int32_t rows[GLASS_NO_SUCH_BOUND]", "float *a, *b"])
def test_parser_refuses_fields_it_does_not_know(decl):
    with pytest.raises(AssertionError):
        H.fields(decl, VOCAB, DEFINES)

