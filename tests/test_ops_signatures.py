"""ops.SIGNATURES and ops.ConvDesc against include/glass_ops.h: the ctypes side of the diagnostic ABI is written by hand, the header is
what the library is compiled from.  Text only: no GPU, no built library.  The header reader is tests/abi_header.py."""
import ctypes as C

import pytest

import abi_header as H
from clip_glass_amd import ops

# what glass_ops.h is known to use: the scalars, [const] T* (and T name[n] as a parameter), an out string and the conv descriptor
VOCAB = H.vocabulary({"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double},
                     {"char*": C.c_char_p, "const glass_conv_desc*": C.POINTER(ops.ConvDesc)})


def prototypes():
    protos, returns = H.prototypes(H.header("glass_ops.h"), VOCAB)
    assert set(returns.values()) == {C.c_int}, "every function of glass_ops.h returns int: %s" % returns
    return protos


def test_signature_table_lists_exactly_the_declared_functions():
    protos = prototypes()
    assert len(protos) >= 60
    assert sorted(ops.SIGNATURES) == sorted(protos)


def test_every_signature_matches_its_prototype():
    wrong = {name: (ops.SIGNATURES.get(name), args) for name, args in prototypes().items() if ops.SIGNATURES.get(name) != args}
    assert not wrong, "ops.SIGNATURES disagrees with include/glass_ops.h (table, header): %s" % wrong


def test_conv_desc_matches_the_struct():
    fields = H.struct_fields(H.header("glass_ops.h"), "glass_conv_desc", VOCAB)
    assert len(fields) >= 47
    assert [(n, t) for n, t in ops.ConvDesc._fields_] == fields


@pytest.mark.parametrize("text", ["int32_t", "const float** x", "size_t n", "const char* s", "glass_conv_desc* d", "float (*f)", "int32_t x, y"])
def test_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(AssertionError):
        H.parameter(text, VOCAB)
