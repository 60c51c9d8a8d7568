"""cim_amd/_abi.py: the parser that turns include/cim_hip.h into the ctypes binding.  Its grammar on a synthetic header, its
refusals, and - the independent check - every struct layout and constant of the real header against the C compiler."""
import ctypes
import os
import re
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_void_p

import pytest

from cim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cim_hip.h")

SYNTHETIC = r"""
/* a comment that holds a declaration: int t_ghost(int a);
 * and a struct: typedef struct { int x; } t_ghost_t; */
#ifndef T_H
#define T_H
#include <stdint.h>
#define A (1 << 4)       /* = 16 */
#define B (A / 3 + 0x10) // = 21: C's division truncates
#ifdef __cplusplus
extern "C" {
#endif
const char* t_error(void);
typedef struct t_item {
    const float* p; int32_t a, b;      /* several declarators per type */
    float w[3];
    const float* q[3];
    uint16_t h, *hp;                   /* the star belongs to ITS declarator */
} t_item;
typedef struct { int32_t n; double d; t_item item[A]; uint8_t grid[2][3]; int64_t tail; } t_args;
long long t_bytes(long long n, double scale,
                  const float* x,
                  void* stream);
int t_run(const t_args* args, const struct t_item* one, int n, float eps, const unsigned char* mask, uint8_t flag, int64_t big);
#ifdef __cplusplus
}
#endif
#endif
"""


def _layout(s):
    return [(name, getattr(s, name).offset, getattr(s, name).size) for name, _ in s._fields_], ctypes.sizeof(s)


def test_grammar_on_a_synthetic_header():
    functions, structs, constants = _abi.parse(SYNTHETIC)
    assert constants == {"A": 16, "B": 21}                                      # (the guard `#define T_H` defines no value)
    assert functions == {
        "t_error": (c_char_p, []),
        "t_bytes": (c_longlong, [c_longlong, c_double, c_void_p, c_void_p]),
        "t_run": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, ctypes.c_uint8, ctypes.c_int64])}
    assert list(structs) == ["t_item", "t_args"]
    item, args = structs["t_item"], structs["t_args"]
    assert issubclass(item, ctypes.Structure) and item.__name__ == "t_item"
    assert [(n, t) for n, t in item._fields_] == [
        ("p", c_void_p), ("a", ctypes.c_int32), ("b", ctypes.c_int32), ("w", c_float * 3), ("q", c_void_p * 3),
        ("h", ctypes.c_uint16), ("hp", c_void_p)]
    assert _layout(item) == ([("p", 0, 8), ("a", 8, 4), ("b", 12, 4), ("w", 16, 12), ("q", 32, 24), ("h", 56, 2), ("hp", 64, 8)], 72)
    assert [(n, t) for n, t in args._fields_] == [
        ("n", ctypes.c_int32), ("d", c_double), ("item", item * 16), ("grid", (ctypes.c_uint8 * 3) * 2), ("tail", ctypes.c_int64)]
    assert _layout(args) == ([("n", 0, 4), ("d", 8, 8), ("item", 16, 1152), ("grid", 1168, 6), ("tail", 1176, 8)], 1184)
    a = args()
    a.item[15].w[2], a.grid[1][2] = 0.5, 7                                      # dimensions in C's order: grid is 2 rows of 3
    assert a.item[15].w[2] == 0.5 and a.grid[1][2] == 7


REFUSED = {
    "an unknown type": ("int t_f(size_t n);", "t_f"),
    "a pointer to an unknown type": ("int t_f(const t_other* p);", "t_f"),
    "a bare `unsigned`": ("int t_f(unsigned n);", "t_f"),
    "an unknown return type": ("float t_f(int n);", "t_f"),
    "an unknown field type": ("typedef struct { int a; short b; } t_s;", "t_s"),
    "a by-value struct parameter": ("typedef struct { int a; } t_s;\nint t_f(t_s s, int n);", "t_f"),
    "a function pointer parameter": ("int t_f(int (*cb)(int), int n);", "t_f"),
    "a function pointer field": ("typedef struct { int a; void (*cb)(int); } t_s;", "t_s"),
    "a bit-field": ("typedef struct { int a : 3; int b; } t_s;", "t_s"),
    "a macro that is no integer": ("#define T_X sizeof(int)\nint t_f(int n);", "T_X"),
    "a macro over an unknown macro": ("#define T_X (T_Y + 1)\nint t_f(int n);", "T_X"),
    "a function-like macro": ("#define T_X(a) ((a) + 1)\nint t_f(int n);", "T_X"),
    "an array sized by an unknown macro": ("typedef struct { float w[T_N]; } t_s;", "t_s"),
    "an unnamed parameter": ("int t_f(int, float x);", "t_f"),
    "an array parameter": ("int t_f(float x[3]);", "t_f"),
    "a nested anonymous struct": ("typedef struct { struct { int a; } in; int b; } t_s;", "typedef"),
    "a variable": ("extern int t_count;", "t_count"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refuses_what_it_does_not_understand(what):
    """Never a guess, never c_int by default: the error names the declaration."""
    text, named = REFUSED[what]
    with pytest.raises(_abi.AbiError, match=named):
        _abi.parse("#include <stdint.h>\n" + text + "\n")


def test_parser_is_standard_library_only():
    src = open(os.path.join(REPO, "cim_amd", "_abi.py")).read()
    assert sorted(re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)) == ["ctypes", "re"]


def test_binding_is_the_header():
    from cim_amd import _lib
    functions, structs, constants = _abi.parse(open(HEADER).read())
    assert len(functions) >= 95 and len(structs) == 8
    assert _lib.SIGNATURES == {n: a for n, (_, a) in functions.items() if n not in ("cim_last_error", "cim_abi_version")}
    assert functions["cim_last_error"] == (c_char_p, []) and functions["cim_abi_version"] == (c_int, [])
    assert {_layout(s) == _layout(_lib.STRUCTS[n]) for n, s in structs.items()} == {True} and constants == _lib.CONSTANTS
    longs = {n for n, (r, _) in functions.items() if r is c_longlong}
    counts = _lib.VALUE_RETURNING - longs
    assert longs <= _lib.VALUE_RETURNING and len(counts) == 7 and all(functions[n][0] is c_int for n in counts)
    assert _lib.PURE <= _lib.VALUE_RETURNING
    lib = _lib.load()
    for name, (restype, argtypes) in functions.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name
    with pytest.raises(_lib.CimHipError, match="no_such_header.h"):
        _lib.parse_header(os.path.join(REPO, "include", "no_such_header.h"))


def test_experiments_binding_is_its_header():
    from experiments import _lib as xlib
    functions, structs, constants = _abi.parse(open(os.path.join(REPO, "experiments", "include", "cim_exp.h")).read())
    assert len(functions) == 19 and not structs and not constants
    assert xlib.SIGNATURES == {n: a for n, (_, a) in functions.items()} and xlib.VALUE_RETURNING <= set(functions)
    assert all(r is c_int for r, _ in functions.values())


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What the C compiler says about the real header: sizeof / offsetof / field size of every struct the parser found, the value
    of every macro it found.  One host-only C program, built with the compiler cim_amd/build.py builds the library with."""
    _, structs, constants = _abi.parse(open(HEADER).read())
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cim_hip.h"', 'int main(void) {']
    for name, s in structs.items():
        lines.append('    printf("S %s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in s._fields_:
            lines.append('    printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
    for name in constants:
        lines.append('    printf("C %s %%lld\\n", (long long)(%s));' % (name, name))
    lines += ['    return 0;', '}', '']
    d = tmp_path_factory.mktemp("abi")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no ROCm compiler at %s: cim_amd/build.py cannot build the library either" % hipcc
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), src, "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes, fields, values = {}, {}, {}
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "S":
            sizes[rest[0]] = int(rest[1])
        elif kind == "F":
            fields.setdefault(rest[0], []).append((rest[1], int(rest[2]), int(rest[3])))
        else:
            values[rest[0]] = int(rest[1])
    return structs, constants, sizes, fields, values


def test_struct_layouts_are_the_compilers(compiled):
    structs, _, sizes, fields, _ = compiled
    assert set(structs) == {"cim_mining_layer", "cim_mining_args", "cim_bn_part_desc", "cim_wt_desc", "cim_loss_args",
                            "cim_sgd_tensor", "cim_sgd_chunk", "cim_adam_tensor"}
    for name, s in structs.items():
        assert _layout(s) == (fields[name], sizes[name]), name


def test_constants_are_the_compilers(compiled):
    _, constants, _, _, values = compiled
    assert len(constants) >= 21 and constants == values
