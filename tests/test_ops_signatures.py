"""ops.SIGNATURES and ops.ConvDesc against include/glass_ops.h: the ctypes side of the diagnostic ABI is written by hand, the header is
what the library is compiled from.  Text only: no GPU, no built library."""
import ctypes as C
import os
import re

import pytest

from clip_glass_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
POINTEES = {"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double}      # [const] T*, and T name[n] as a parameter


def header():
    src = open(os.path.join(ROOT, "include", "glass_ops.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def ctype(const, base, star, array=""):
    """The ctypes type of one C declaration `[const] base [*] name [[n]]`; anything the header is not known to use is an error."""
    if not star and not array:
        assert base in SCALARS and not const, "unrecognised type: %s%s" % (const, base)
        return SCALARS[base]
    assert not (star and array), "unrecognised declarator"
    if base == "char" and not const:
        return C.c_char_p
    if base == "glass_conv_desc" and const:
        return C.POINTER(ops.ConvDesc)
    assert base in POINTEES, "unrecognised pointer type: %s%s*" % (const, base)
    return C.POINTER(POINTEES[base])


def parameter(text):
    m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*\w+\s*(\[\d+\])?", text.strip())
    assert m, "unrecognised parameter: %r" % text
    return ctype(m.group(1) or "", m.group(2), m.group(3), m.group(4) or "")


def prototypes(src):
    """{name: [ctypes of the parameters]} of every `int glass_*(...);`."""
    found = {name: [parameter(p) for p in params.split(",")] for name, params in re.findall(r"\bint\s+(glass_\w+)\s*\(([^()]*)\)\s*;", src)}
    called = set(re.findall(r"\b(glass_\w+)\s*\(", src))
    assert set(found) == called, "declared, but not as `int name(...);`: %s" % sorted(called ^ set(found))
    return found


def struct_fields(src, name):
    """[(field, ctype)] of `typedef struct name { ... } name;`, lines with several declarators expanded."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)", decl)
        assert m, "unrecognised field: %r" % decl
        names = [n.strip() for n in m.group(4).split(",")]
        assert not m.group(3) or len(names) == 1, "several pointer declarators on one line: %r" % decl
        fields += [(n, ctype(m.group(1) or "", m.group(2), m.group(3))) for n in names]
    return fields


def test_signature_table_lists_exactly_the_declared_functions():
    protos = prototypes(header())
    assert len(protos) >= 60
    assert sorted(ops.SIGNATURES) == sorted(protos)


def test_every_signature_matches_its_prototype():
    wrong = {name: (ops.SIGNATURES.get(name), args) for name, args in prototypes(header()).items() if ops.SIGNATURES.get(name) != args}
    assert not wrong, "ops.SIGNATURES disagrees with include/glass_ops.h (table, header): %s" % wrong


def test_conv_desc_matches_the_struct():
    fields = struct_fields(header(), "glass_conv_desc")
    assert len(fields) >= 47
    assert [(n, t) for n, t in ops.ConvDesc._fields_] == fields


@pytest.mark.parametrize("text", ["int32_t", "const float** x", "size_t n", "const char* s", "glass_conv_desc* d", "float (*f)", "int32_t x, y"])
def test_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(AssertionError):
        parameter(text)
