"""The C ABI of a header as ctypes: prototypes, `typedef struct`s and integer `#define`s, read from the header's text.

`parse(text)` understands exactly the C that include/cim_hip.h and experiments/include/cim_exp.h are written in and REFUSES
everything else (AbiError names the declaration): a binding that guessed a type would hand an integer to a kernel as a device
pointer.  Standard library only - tests/test_abi_cpu.py checks every struct layout and constant against the C compiler."""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}
SCALARS.update(("%sint%d_t" % (u, b), getattr(ctypes, "c_%sint%d" % (u, b))) for u in ("", "u") for b in (8, 16, 32, 64))
_POINTEES = ("void", "char", "unsigned char")       # besides the scalars and the structs: what a pointer may point to

_DECLARATION = re.compile(r'\s*(?:(extern\s*"C"\s*\{|\})'                                # the C++ guard's two halves
                          r'|typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;'        # typedef struct [tag] { fields } name;
                          r'|([^;{}]+);)')                                               # anything else up to its semicolon
_PROTOTYPE = re.compile(r'(int\b|long\s+long\b|const\s+char\s*\*)\s*(\w+)\s*\((.*)\)', re.S)
_RESTYPES = {"int": ctypes.c_int, "longlong": ctypes.c_longlong, "constchar*": ctypes.c_char_p}      # (spelled without blanks)
_FIRST = re.compile(r'(.+?)\s*\b(\w+)\s*((?:\[[^\]]*\]\s*)*)', re.S)        # type (with its stars), name, [dims]
_NEXT = re.compile(r'(\**)\s*(\w+)\s*((?:\[[^\]]*\]\s*)*)')                 # a further declarator of the same type
_INT_EXPR = re.compile(r'(?:0[xX][0-9a-fA-F]+|\d+|<<|>>|[-+*/%()|&~^]|\s)+')


class AbiError(ValueError):
    pass


def _integer(expr, constants, where):
    """An integer constant expression over literals and earlier macros (C semantics: `/` truncates)."""
    text = re.sub(r'\b[A-Za-z_]\w*\b', lambda m: str(constants.get(m.group(0), m.group(0))), expr)
    text = re.sub(r'\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b', r'\1', text)
    if not text.strip() or not _INT_EXPR.fullmatch(text):
        raise AbiError("%s: `%s` is not an integer expression over known macros" % (where, expr.strip()))
    try:
        return int(eval(text.replace("/", "//"), {"__builtins__": {}}))
    except Exception:
        raise AbiError("%s: `%s` does not evaluate to an integer" % (where, expr.strip()))


def _ctype(spec, pointer, structs, tags, where, by_value_struct):
    """ctypes type of the type specifier `spec` (stars ignored; `pointer`: the declarator is one - every pointer is c_void_p)."""
    base = " ".join(w for w in spec.replace("*", " ").split() if w != "const")
    if pointer:
        if base in SCALARS or base in _POINTEES or base in structs or (base.startswith("struct ") and base[7:] in tags):
            return ctypes.c_void_p
    elif base in SCALARS:
        return SCALARS[base]
    elif base in structs:
        if by_value_struct:
            return structs[base]
        raise AbiError("%s: struct `%s` passed by value" % (where, base))
    raise AbiError("%s: unknown type `%s`" % (where, base))


def _dims(t, dims, constants, where):
    for d in reversed(re.findall(r'\[([^\]]*)\]', dims)):
        t = t * _integer(d, constants, where)
    return t


def _parameter(text, structs, tags, where):
    m = _FIRST.fullmatch(text.strip())
    if not m or m.group(3):
        raise AbiError("%s: parameter `%s` is not `type name`" % (where, " ".join(text.split())))
    return _ctype(m.group(1), "*" in m.group(1), structs, tags, where, by_value_struct=False)


def _fields(body, structs, tags, constants, where):
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        at = "%s, field `%s`" % (where, decl)
        if ":" in decl:
            raise AbiError("%s: bit-field" % at)
        if "(" in decl:
            raise AbiError("%s: function pointer" % at)
        first, *more = decl.split(",")
        m = _FIRST.fullmatch(first.strip())
        if not m:
            raise AbiError("%s: not `type name[, name ...]`" % at)
        spec, declarators = m.group(1), [("*" in m.group(1), m.group(2), m.group(3))]       # (a star binds to ITS declarator only)
        for d in more:
            n = _NEXT.fullmatch(d.strip())
            if not n:
                raise AbiError("%s: declarator `%s`" % (at, d.strip()))
            declarators.append((bool(n.group(1)), n.group(2), n.group(3)))
        fields += [(name, _dims(_ctype(spec, pointer, structs, tags, at, True), dims, constants, at)) for pointer, name, dims in declarators]
    return fields


def parse(text):
    """-> (functions: name -> (restype, [argtypes]), structs: name -> ctypes.Structure subclass, constants: name -> int)"""
    functions, structs, constants, tags = {}, {}, {}, set()
    text = re.sub(r'/\*.*?\*/|//[^\n]*', " ", text.replace("\\\n", " "), flags=re.S)
    code = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r'\s*#\s*define\s+(\w+)(.*)', line)
        if m and m.group(2).startswith("("):
            raise AbiError("#define %s: function-like macro" % m.group(1))
        if m and m.group(2).strip():                        # (`#define GUARD_H` alone defines no value)
            constants[m.group(1)] = _integer(m.group(2), constants, "#define %s" % m.group(1))
    text, pos = "\n".join(code).rstrip(), 0
    while pos < len(text):
        m = _DECLARATION.match(text, pos)
        if not m:
            raise AbiError("unrecognised declaration at `%s`" % " ".join(text[pos:].split())[:80])
        pos = m.end()
        if m.group(1):
            continue
        if m.group(4):
            name = m.group(4)
            fields = _fields(m.group(3), structs, tags, constants, "struct %s" % name)
            structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
            tags.add(m.group(2))
            continue
        decl = " ".join(m.group(5).split())
        p = _PROTOTYPE.fullmatch(decl)
        if not p:
            raise AbiError("unrecognised declaration `%s`" % decl)
        where, args = "%s()" % p.group(2), p.group(3).strip()
        if "(" in args or ")" in args:
            raise AbiError("%s: function pointer in `%s`" % (where, decl))
        argtypes = [] if args == "void" else [_parameter(a, structs, tags, where) for a in args.split(",")]
        functions[p.group(2)] = (_RESTYPES["".join(p.group(1).split())], argtypes)
    return functions, structs, constants
