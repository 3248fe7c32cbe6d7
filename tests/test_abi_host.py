"""The ctypes binding is derived from include/textboost_hip.h (textboost_amd/_abi.py): struct layouts against the C compiler, every prototype
bound with the right arity and descriptor classes, the parser's behaviour on synthetic header text, and the constants _lib.py spells out."""
import ctypes as C
import os
import re
import subprocess

import pytest

from textboost_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "textboost_hip.h")
DESCS = {"tb_gemm_desc": _lib.GemmDesc, "tb_attn_desc": _lib.AttnDesc, "tb_ff_desc": _lib.FfDesc, "tb_chain_desc": _lib.ChainDesc,
         "tb_opt_desc": _lib.OptDesc}


@pytest.fixture(scope="module")
def protos():
    """{name: [parameter text, ...]} read from the comment-stripped header, independently of the parser under test"""
    text = _abi.strip_comments(open(HEADER).read())
    found = re.findall(r"\b(tb_[a-z0-9_]+)\s*\(([^()]*)\)", text)
    assert len(found) == len({n for n, _ in found})
    return {n: [] if a.strip() == "void" else [p.strip() for p in a.split(",")] for n, a in found}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from textboost_amd.build import _hipcc
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "textboost_hip.h"', "int main(void) {"]
    for cname, cls in DESCS.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = tmp_path / "layout"
    subprocess.run([_hipcc(), "-x", "c", str(src), "-I", os.path.dirname(HEADER), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in DESCS.items():
        want[cname] = str(C.sizeof(cls))
        want.update({f"{cname}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert [C.sizeof(c) for c in DESCS.values()] == [360, 208, 304, 160, 232]


def test_every_prototype_is_bound(protos):
    assert set(protos) == set(_lib._SIGS) and len(protos) >= 115
    for name, params in protos.items():
        argtypes, _ = _lib._SIGS[name]
        assert len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            m = re.match(r"const (tb_\w+_desc)\s*\*", p)
            if m:
                assert t is C.POINTER(DESCS[m.group(1)]), (name, p)
            else:
                assert "_desc" not in p and not (isinstance(t, type) and issubclass(t, C._Pointer)), (name, p)
        # the stream is the last parameter of every entry point that takes one, no exception: ops._launch appends it
        assert not any(p.startswith("tb_stream_t") for p in params[:-1]), name
        if params and params[-1].startswith("tb_stream_t"):
            assert argtypes[-1] is C.c_void_p
    assert _lib._SIGS["tb_last_hip_error"] == ([], C.c_char_p)
    assert _lib._SIGS["tb_gemm_last_config"] == ([C.c_void_p], None)
    assert _lib._SIGS["tb_attention_fp8_ws_bytes"] == ([C.c_int] * 3, C.c_int64)
    assert _lib._SIGS["tb_scaler_update"][0][:4] == [C.c_void_p, C.c_float, C.c_double, C.c_double]
    # the one host pointer the callers set with ctypes.pointer(): a c_void_p field would refuse it
    assert dict(_lib.GemmDesc._fields_)["split_out"] is C.POINTER(C.c_int32)
    _lib.GemmDesc().split_out = C.pointer(C.c_int32(1))


SYNTHETIC = """
/* a comment with ; and ( and ) and a call tb_fake(123); in it */
#ifndef X_H
#define X_H
#include <stdint.h>
#define TB_IMG_THING 7 /* trailing ; comment */
#ifdef __cplusplus
extern "C" {
#endif
typedef void* tb_stream_t; /* hipStream_t */
enum { TB_ONE = 1, /* ( */ TB_TWO = 2 };
typedef struct tb_tagged_desc {
  int64_t M; int32_t B, Hin, Win;   /* multi-declarator; with a ; */
  const void* A; float alpha;
  int32_t* split_out; uint32_t* sync;
} tb_tagged_desc;
typedef struct {
  float* state; double beta1, beta2;
} tb_untagged_desc;
/* between declarations: tb_between(1, 2); */
int tb_run(const tb_tagged_desc* d, const void* const* p /* tb_inside(3); */, int n, tb_stream_t stream);
int64_t tb_tail(const tb_untagged_desc* d, const float* x, uint8_t* m, const int64_t* ids, int* slots, const double* a);
void tb_nothing(void);
const char* tb_text(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_synthetic_header_text():
    structs, sigs, consts = _abi.parse(SYNTHETIC)
    assert consts == {"TB_IMG_THING": 7, "TB_ONE": 1, "TB_TWO": 2}
    tagged, untagged = structs["tb_tagged_desc"], structs["tb_untagged_desc"]
    assert tagged._fields_ == [("M", C.c_int64), ("B", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("A", C.c_void_p),
                               ("alpha", C.c_float), ("split_out", C.POINTER(C.c_int32)), ("sync", C.c_void_p)]
    assert untagged._fields_ == [("state", C.c_void_p), ("beta1", C.c_double), ("beta2", C.c_double)]
    assert sigs == {"tb_run": ([C.POINTER(tagged), C.c_void_p, C.c_int, C.c_void_p], C.c_int),
                    "tb_tail": ([C.POINTER(untagged)] + [C.c_void_p] * 5, C.c_int64),
                    "tb_nothing": ([], None),
                    "tb_text": ([], C.c_char_p)}


@pytest.mark.parametrize("bad, what", [
    ("int tb_f(size_t n);", "size_t"),                                           # a type the table does not know
    ("int tb_f(const size_t* n);", "size_t"),                                    # ... also behind a pointer
    ("typedef struct tb_s { int a; } tb_s; int tb_f(tb_s d);", "by value"),      # a struct passed by value
    ("typedef struct tb_s { int a[4]; } tb_s;", "int a[4]"),                     # an array field
    ("typedef struct tb_s { float *a, *b; } tb_s;", "declarators"),              # the star belongs to the type
    ("int tb_f(int);", "int tb_f(int)"),                                         # an unnamed parameter
    ("enum { TB_A, TB_B };", "TB_A"),                                            # an enumerator without a value
    ("static inline int tb_f(int n) { return n; }", "classify"),                 # a definition
    ("int tb_ok(int n); struct tb_s;", "classify"),                              # a statement the grammar has no rule for
])
def test_parser_raises_on_what_it_does_not_know(bad, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        _abi.parse('extern "C" {\ntypedef void* tb_stream_t;\n' + bad + "\n}\n")


def test_missing_header_names_the_path(tmp_path):
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "nope.h"))):
        _abi.load(str(tmp_path / "nope.h"))


def test_constants_equal_the_header():
    consts = _abi.load()[2]
    assert len(consts) >= 32 and all(n.startswith("TB_") for n in consts)
    assert {n for n in consts if n.startswith("TB_IMG_")} == {"TB_IMG_LANCZOS", "TB_IMG_BICUBIC", "TB_IMG_BILINEAR"}
    for name, value in consts.items():
        py = name if name in ("TB_F16", "TB_F32") else name[3:]
        assert getattr(_lib, py, None) == value, f"{name} = {value} in the header, _lib.{py} = {getattr(_lib, py, None)}"
