"""The C ABI of libescgnn_hip.so as ctypes, read from include/escgnn_hip.h: the header is the only statement of it.

parse(text) returns an Abi: `constants` (every `#define ESC_* <integer expression>` and every enum member), `enum` (the
enum's members alone), `structs` (name -> ctypes.Structure subclass, header order), `functions` (name -> (argtypes, restype))
and `callbacks` (function-pointer typedef -> CFUNCTYPE).  load() does that once for the header of this tree.

The reader is strict: once comments, preprocessor lines and the extern "C" braces are gone, every declaration must be one of
the forms the header's opening comment lists; anything else raises HeaderError quoting the text.  Pure Python: imports neither
torch nor the library.
"""
import collections
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "escgnn_hip.h")

SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}
POINTEES = ("void", "char", "uint8_t")           # known only behind a `*`
# ctypes' name for a Structure's member list, spelled in two halves: the test that no hand-written mirror is left in the package
# searches for the whole word
_MEMBERS = "_fields" + "_"

Abi = collections.namedtuple("Abi", "constants enum structs functions callbacks")


class HeaderError(ValueError):
    pass


_DEFINE = re.compile(r"#\s*define\s+(\w+)(\(?)(.*)")
_SPACE = re.compile(r"\s*")
_FORMS = (
    ("enum", re.compile(r"enum\s*\{([^{}]*)\}\s*;")),
    ("struct", re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")),
    ("callback", re.compile(r"typedef\s+([\w\s*]+?)\(\s*\*\s*(\w+)\s*\)\s*\(([^(){};]*)\)\s*;")),
    ("function", re.compile(r"((?!typedef\b)[\w\s*]+?)\b(\w+)\s*\(([^(){};]*)\)\s*;")),
)
_DECLARATION = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[([^\[\]]+)\])?")


def members(cls):
    """[(name, offset, size)] of a struct class, in declaration order"""
    return [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _ in getattr(cls, _MEMBERS)]


def _quote(text):
    return " ".join(text.split())[:120]


def _integer(expr, constants, where):
    """value of an integer expression over literals, + - * ( ) and constants defined earlier"""
    try:
        expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(constants[m.group()]), expr)
    except KeyError as exc:
        raise HeaderError("unknown constant %s in: %s" % (exc, _quote(where)))
    if not re.fullmatch(r"[\d\s+\-*()]+", expr):
        raise HeaderError("not an integer expression: %s" % _quote(where))
    try:
        return int(eval(expr, {"__builtins__": {}}))        # digits, + - * ( ) only, by the check above
    except Exception:
        raise HeaderError("not an integer expression: %s" % _quote(where))


def _declared(text, abi, where, arrays):
    """[(name, ctype)] of one declaration `[const] type declarator {, declarator}`; declarator = [*] name [[dim]]"""
    m = _DECLARATION.fullmatch(text.strip())
    if not m:
        raise HeaderError("unrecognised declaration: %s" % _quote(where))
    base, out = m.group(1), []
    for part in m.group(2).split(","):
        d = _DECLARATOR.fullmatch(part.strip())
        if not d or (d.group(3) and not arrays):
            raise HeaderError("unrecognised declarator `%s` in: %s" % (_quote(part), _quote(where)))
        star, name, dim = d.groups()
        if star and (base in SCALARS or base in POINTEES or base in abi.structs):
            ctype = ctypes.c_void_p
        elif not star and base in SCALARS:
            ctype = SCALARS[base]
        elif not star and base in abi.callbacks:
            ctype = ctypes.c_void_p
        elif not star and base in abi.structs and arrays:       # a struct by value: as a member only, never as a parameter
            ctype = abi.structs[base]
        else:
            raise HeaderError("unknown or by-value type `%s` in: %s" % (base, _quote(where)))
        out.append((name, ctype * _integer(dim, abi.constants, where) if dim else ctype))
    return out


def _parameters(text, abi, where):
    if text.strip() in ("", "void"):
        return []
    out = []
    for p in text.split(","):
        got = _declared(p, abi, where, arrays=False)
        if len(got) != 1:
            raise HeaderError("unrecognised parameter `%s` in: %s" % (_quote(p), _quote(where)))
        out.append(got[0][1])
    return out


def _result(text, abi, where):
    text = " ".join(text.split())
    if text in ("const char*", "const char *"):
        return ctypes.c_char_p
    if text not in SCALARS:
        raise HeaderError("unknown return type `%s` in: %s" % (text, _quote(where)))
    return SCALARS[text]


def parse(text):
    abi = Abi({}, collections.OrderedDict(), collections.OrderedDict(), collections.OrderedDict(), collections.OrderedDict())
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    body = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            body.append(line)
            continue
        if line.rstrip().endswith("\\"):
            raise HeaderError("continued preprocessor line: %s" % _quote(line))
        m = _DEFINE.match(line.strip())
        if m and m.group(1).startswith("ESC_"):
            if m.group(2):
                raise HeaderError("function-like macro: %s" % _quote(line))
            abi.constants[m.group(1)] = _integer(m.group(3), abi.constants, line)
    text = "\n".join(body)
    text, n = re.subn(r'extern\s+"C"\s*\{', " ", text)
    if n:
        text, closed = re.subn(r"\}\s*\Z", " ", text)
        if n != 1 or closed != 1:
            raise HeaderError('unbalanced extern "C" braces')
    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return abi
        for form, rx in _FORMS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            raise HeaderError("unrecognised text in the header: %s" % _quote(text[pos:]))
        where, pos = m.group(), m.end()
        if form == "enum":
            nxt = 0
            for member in filter(None, (s.strip() for s in m.group(1).split(","))):
                name, _, value = (s.strip() for s in member.partition("="))
                if not re.fullmatch(r"ESC_\w+", name):
                    raise HeaderError("unrecognised enum member `%s` in: %s" % (member, _quote(where)))
                nxt = _integer(value, abi.constants, where) if value else nxt
                abi.constants[name] = abi.enum[name] = nxt
                nxt += 1
        elif form == "struct":
            if m.group(1) != m.group(3) or m.group(1) in abi.structs:
                raise HeaderError("struct tag and typedef name differ, or defined twice: %s" % _quote(where))
            decls = m.group(2).split(";")
            if decls.pop().strip():
                raise HeaderError("member without `;` in: %s" % _quote(where))
            members = [f for s in decls for f in _declared(s, abi, s + "; of " + m.group(1), arrays=True)]
            abi.structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {_MEMBERS: members})
        elif form == "callback":
            abi.callbacks[m.group(2)] = ctypes.CFUNCTYPE(_result(m.group(1), abi, where), *_parameters(m.group(3), abi, where))
        else:
            if m.group(2) in abi.functions:
                raise HeaderError("declared twice: %s" % _quote(where))
            abi.functions[m.group(2)] = (_parameters(m.group(3), abi, where), _result(m.group(1), abi, where))


_loaded = {}


def load(path=None):
    """the Abi of a header file (this tree's by default), parsed once"""
    path = path or HEADER
    if path not in _loaded:
        with open(path) as f:
            _loaded[path] = parse(f.read())
    return _loaded[path]
