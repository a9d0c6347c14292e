"""A reader of the project's C headers (include/glass.h, include/glass_ops.h) for the tests that hold the hand-written ctypes tables against
them.  Text only: no GPU, no built library.  A header is read with a vocabulary — {C type as written: ctypes type} — that lists what that
header is known to use; a declaration outside it, or in a form the reader does not know, is an assertion error, never a guess."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int, "void": None, "const char*": C.c_char_p}
STARS = r"(?:\*\s*(?:const\b\s*)?)+"
DECLARATOR = r"\w+(?:\s*\[\w+\])*"


def spelled(const, base, stars):
    """One spelling per C type: `const float * const *` and `const float* const*` are the same vocabulary entry."""
    return ("const " if const else "") + base + re.sub(r"\s+", "", stars).replace("*const", "* const")


def canonical(text):
    return spelled(*re.fullmatch(r"(const\s+)?(\w+)\s*(.*)", text.strip()).groups())


def vocabulary(pointees, extra):
    """The scalars; `T*` and `const T*` for each pointee; and the header's own types, spelled as the header spells them."""
    vocab = dict(SCALARS)
    for name, t in pointees.items():
        vocab[name + "*"] = vocab["const " + name + "*"] = C.POINTER(t)
    vocab.update({canonical(k): t for k, t in extra.items()})
    return vocab


def header(name):
    """include/<name> without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def defines(src):
    """{NAME: value} of every `#define NAME <integer>`."""
    return {name: int(value) for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", src, flags=re.M)}


def lookup(vocab, const, base, stars):
    key = spelled(const, base, stars)
    assert key in vocab, "unrecognised type: %s" % key
    return vocab[key]


def parameter(text, vocab):
    """The ctypes type of one parameter `[const] base [*...] name [[n]]`; an array parameter is a pointer to its element."""
    m = re.fullmatch(r"(const\s+)?(\w+)(\s*%s\s*|\s+)(\w+)\s*(\[\w+\])?" % STARS, text.strip())
    assert m, "unrecognised parameter: %r" % text
    const, base, stars, _, array = m.groups()
    assert not (stars.strip() and array), "unrecognised declarator: %r" % text
    return lookup(vocab, const, base, stars.strip() + ("*" if array else ""))


def prototypes(src, vocab):
    """({name: [ctypes of the parameters]}, {name: ctypes return type}) of every `<int | void | const char*> glass_*(...);`."""
    args, returns = {}, {}
    for ret, name, params in re.findall(r"\b(int|void|const\s+char\s*\*)\s*(glass_\w+)\s*\(([^()]*)\)\s*;", src):
        args[name] = [] if params.strip() == "void" else [parameter(p, vocab) for p in params.split(",")]
        returns[name] = RETURNS[canonical(ret)]
    called = set(re.findall(r"\b(glass_\w+)\s*\(", src))
    assert set(args) == called, "declared, but not as `int | void | const char* name(...);`: %s" % sorted(called ^ set(args))
    return args, returns


def fields(decl, vocab, bounds={}):
    """[(field, ctype)] of one struct member declaration: several declarators expanded, `name[N]` and `name[N][M]` as ctypes arrays with
    N an integer or one of `bounds` (the header's #defines)."""
    m = re.fullmatch(r"(const\s+)?(\w+)(\s*%s\s*|\s+)(%s(?:\s*,\s*%s)*)" % (STARS, DECLARATOR, DECLARATOR), decl.strip())
    assert m, "unrecognised field: %r" % decl
    const, base, stars, declarators = m.groups()
    declarators = [d.strip() for d in declarators.split(",")]
    assert not stars.strip() or len(declarators) == 1, "several pointer declarators on one line: %r" % decl
    out = []
    for d in declarators:
        t = lookup(vocab, const, base, stars.strip())
        for n in reversed(re.findall(r"\[(\w+)\]", d)):
            assert n.isdigit() or n in bounds, "unknown array bound %r: %r" % (n, decl)
            t = t * (int(n) if n.isdigit() else bounds[n])
        out.append((re.match(r"\w+", d).group(0), t))
    return out


def struct_fields(src, name, vocab):
    """[(field, ctype)] of `typedef struct name { ... } name;`."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    bounds = defines(src)
    return [f for decl in filter(None, (d.strip() for d in body.split(";"))) for f in fields(decl, vocab, bounds)]
