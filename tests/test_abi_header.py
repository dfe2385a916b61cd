"""_lib's reader of include/gcnk.h and the family headers it includes, without a GPU: the exact ctypes result on a
synthetic header that holds every form the real ones use, the loud failures, an umbrella with a family header, and
the real headers against test_abi.py's own regex and the library."""
import collections
import ctypes as C
import os

import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, record

import test_abi

SYNTHETIC = """\
/* the C-ABI; gcnk_in_a_comment(int x); is no declaration */
#ifndef GCNK_H_
#define GCNK_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GCNK_ABI_VERSION 13
#define GCNK_EARG (-1)
#define GCNK_EPI_BIAS 1   /* + bias[col] (layer.py:110); */
#define GCNK_MASK 0x10
#define GCNK_ROW_WORDS(P) (3 * (P) + 3)
const char* gcnk_last_error(void);
typedef struct gcnk_x {
  const float* p;              /* device */
  int32_t M, F;                /* rows, width */
  int32_t hdr[4];
  int64_t numel;
} gcnk_x;
typedef struct gcnk_y { gcnk_x a, b; uint32_t flags; double best; } gcnk_y;   /* 96 bytes */
int gcnk_open(const char* path, const void* plan, uint8_t* mask,
              const gcnk_x* t /* host */, int64_t ld,
              uint64_t seed, float scale, void* stream);
int32_t gcnk_count(const gcnk_y* y, uint32_t word, double p);
#ifdef __cplusplus
}
#endif
#endif /* GCNK_H_ */
"""


def test_synthetic_header_gives_exactly_these_ctypes():
    sig, structs, const = _lib.parse_header(SYNTHETIC)
    vp = C.c_void_p
    assert sig == {"gcnk_last_error": (C.c_char_p, []),
                   "gcnk_open": (C.c_int, [C.c_char_p, vp, vp, vp, C.c_int64, C.c_uint64, C.c_float, vp]),
                   "gcnk_count": (C.c_int32, [vp, C.c_uint32, C.c_double])}
    assert const == {"ABI_VERSION": 13, "EARG": -1, "EPI_BIAS": 1, "MASK": 16}   # no ROW_WORDS, no H_
    assert list(structs) == ["gcnk_x", "gcnk_y"]
    x, y = structs["gcnk_x"], structs["gcnk_y"]
    assert issubclass(x, C.Structure) and x.__name__ == "gcnk_x"
    assert x._fields_ == [("p", vp), ("M", C.c_int32), ("F", C.c_int32), ("hdr", C.c_int32 * 4), ("numel", C.c_int64)]
    assert y._fields_ == [("a", x), ("b", x), ("flags", C.c_uint32), ("best", C.c_double)]
    assert [(getattr(x, f).offset, getattr(x, f).size) for f, _ in x._fields_] == [(0, 8), (8, 4), (12, 4), (16, 16),
                                                                                  (32, 8)]
    assert (C.sizeof(x), C.sizeof(y), y.b.offset, y.flags.offset, y.best.offset) == (40, 96, 40, 80, 88)


def _with(line):
    return SYNTHETIC.replace("int32_t gcnk_count(", line + "\nint32_t gcnk_count(")


@pytest.mark.parametrize("line, named", [
    ("int gcnk_bad(size_t n);", "size_t"),                                   # an unknown type: by value,
    ("int gcnk_bad(const gcnk_z* z);", "gcnk_z"),                            # behind a pointer (a struct not yet seen),
    ("unsigned gcnk_bad(void);", "unsigned"),                                # as the return,
    ("typedef struct gcnk_z { int16_t a; } gcnk_z;", "int16_t"),             # in a struct
    ("int gcnk_bad(int32_t out[4]);", "out[4]"),                             # an array as a parameter
    ("typedef struct gcnk_z { float* a, b; } gcnk_z;", "float* a, b"),       # `b` would be no pointer
    ("int gcnk_half(int32_t a) __attribute__((unused));", "gcnk_half"),      # statements consumed in part only
    ("typedef struct gcnk_z { int32_t a; } gcnk_z, gcnk_w;", "gcnk_z"),
    ("typedef struct gcnk_z { struct { int32_t a; } in; } gcnk_z;", "gcnk_z"),
    ("struct gcnk_forward;", "gcnk_forward"),
    ("int gcnk_inline(void) { return 0; }", "gcnk_inline"),
    ("int other_prefix(void);", "other_prefix"),
    ("#define GCNK_SHIFTED (1 << 3)", "GCNK_SHIFTED"),                       # a constant that is no integer
    ("#define GCNK_ALIAS GCNK_EARG", "GCNK_ALIAS"),
])
def test_what_the_reader_cannot_take_whole_raises_and_names_it(line, named):
    with pytest.raises(RuntimeError, match=r"gcnk\.h") as e:
        _lib.parse_header(_with(line))
    assert named in str(e.value)
    with pytest.raises(RuntimeError, match=r"^gcnk_family\.h: ") as e:      # the header at fault is the one named
        _lib.parse_header(_with(line), "gcnk_family.h")
    assert named in str(e.value)


def test_text_outside_the_extern_block_and_a_missing_header_raise(tmp_path):
    with pytest.raises(RuntimeError, match='extern "C"'):
        _lib.parse_header(SYNTHETIC.replace("#include <stdint.h>", "int gcnk_outside(void);"))
    with pytest.raises(RuntimeError, match='extern "C"'):
        _lib.parse_header("#define GCNK_OK 0\nint gcnk_abi_version(void);\n")
    missing = str(tmp_path / "include" / "gcnk.h")
    with pytest.raises(RuntimeError, match="not found") as e:
        _lib.read_header(missing)
    assert missing in str(e.value)


FAMILY = """\
/* a family header in the same form; it may hold constants and structs of its own */
#ifndef GCNK_FAMILY_H_
#define GCNK_FAMILY_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GCNK_FAMILY_CHUNK 256
typedef struct gcnk_f { int64_t n; } gcnk_f;
int gcnk_family_run(const gcnk_f* f, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def _two_headers(tmp_path, family=FAMILY, include='#include "gcnk_family.h"   /* beside this file */'):
    umbrella = tmp_path / "gcnk.h"
    umbrella.write_text(SYNTHETIC.replace("int32_t gcnk_count(", "// #include \"gcnk_commented_out.h\"\n" + include
                                          + "\nint32_t gcnk_count("))
    if family is not None:
        (tmp_path / "gcnk_family.h").write_text(family)
    return str(umbrella)


def test_an_umbrella_and_the_family_header_it_includes_are_one_binding(tmp_path):
    paths, declared_in, sig, structs, const = _lib.read_headers(_two_headers(tmp_path))
    assert paths == [str(tmp_path / "gcnk.h"), str(tmp_path / "gcnk_family.h")]
    assert declared_in == {"gcnk_last_error": "gcnk.h", "gcnk_open": "gcnk.h", "gcnk_count": "gcnk.h",
                           "gcnk_family_run": "gcnk_family.h"}
    assert list(sig) == list(declared_in) and sig["gcnk_family_run"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert list(structs) == ["gcnk_x", "gcnk_y", "gcnk_f"] and structs["gcnk_f"]._fields_ == [("n", C.c_int64)]
    assert const == {"ABI_VERSION": 13, "EARG": -1, "EPI_BIAS": 1, "MASK": 16, "FAMILY_CHUNK": 256}


@pytest.mark.parametrize("line, named", [("int gcnk_count(void);", "gcnk_count"),             # an entry point,
                                         ("typedef struct gcnk_x { int n; } gcnk_x;", "gcnk_x"),   # a struct,
                                         ("#define GCNK_MASK 0x10", "GCNK_MASK")])                # a constant
def test_a_name_declared_in_two_headers_raises_and_names_both(tmp_path, line, named):
    twice = FAMILY.replace("int gcnk_family_run(", line + "\nint gcnk_family_run(")
    with pytest.raises(RuntimeError) as e:
        _lib.read_headers(_two_headers(tmp_path, twice))
    assert named in str(e.value) and "gcnk_family.h" in str(e.value) and "gcnk.h" in str(e.value).replace(
        "gcnk_family.h", "")


def test_a_named_include_that_does_not_exist_and_a_bad_family_header_raise(tmp_path):
    with pytest.raises(RuntimeError, match="not found") as e:
        _lib.read_headers(_two_headers(tmp_path, family=None))
    assert str(tmp_path / "gcnk_family.h") in str(e.value)
    with pytest.raises(RuntimeError, match=r"^gcnk_family\.h: .*size_t"):
        _lib.read_headers(_two_headers(tmp_path, FAMILY.replace("void* stream", "size_t n")))


def test_real_header_is_read_whole_and_the_public_names_are_its_structs():
    paths, declared_in, sig, structs, const = _lib.read_headers()
    assert [os.path.relpath(p, test_abi.ROOT) for p in paths] == [os.path.join("include", h) for h in (
        "gcnk.h", "gcnk_topic_graph.h", "gcnk_lda.h", "gcnk_text.h")] and paths == _lib.HEADERS
    assert collections.Counter(_lib.DECLARED_IN.values()) == {"gcnk.h": 68, "gcnk_topic_graph.h": 6, "gcnk_lda.h": 14,
                                                              "gcnk_text.h": 7}
    assert declared_in == _lib.DECLARED_IN and list(declared_in) == list(sig)
    assert len(sig) == 95 and set(test_abi._declared_symbols()) == set(sig) == set(_lib.SIGNATURES)
    assert {k: C.sizeof(v) for k, v in structs.items()} == {
        "gcnk_plan_ref": 112, "gcnk_gcn_fwd": 536, "gcnk_gcn_bwd": 440, "gcnk_adam_tensor": 40, "gcnk_epoch_state": 32,
        "gcnk_keep_tensor": 24, "gcnk_keep_state": 16}
    assert len(const) == 41 and all(getattr(_lib, k) == v for k, v in const.items())
    assert _lib.HEADER_PATH == os.path.join(test_abi.ROOT, "include", "gcnk.h") == _lib.HEADERS[0]
    # the module's own tables are one reading of it, and every public struct name is the derived class itself
    assert const == _lib.CONSTANTS and sig == _lib.SIGNATURES
    S = _lib.STRUCTS
    assert _lib.AdamTensor is S["gcnk_adam_tensor"] and _lib.EpochState is S["gcnk_epoch_state"]
    assert _lib.KeepTensor is S["gcnk_keep_tensor"] and _lib.KeepState is S["gcnk_keep_state"]
    assert record.PlanRef is S["gcnk_plan_ref"] and record.GcnFwd is S["gcnk_gcn_fwd"]
    assert record.GcnBwd is S["gcnk_gcn_bwd"] and dict(record.GcnFwd._fields_)["aF"] is record.PlanRef
    assert (record.FACTORED, record.SPMM_PROJ, record.SPMM_GEMM, record.DENSE_AX, record.BWD_AX_DIRECT) == (
        _lib.FWD_FACTORED, _lib.FWD_SPMM_PROJ, _lib.FWD_SPMM_GEMM, _lib.FWD_DENSE_AX, _lib.BWD_AX_DIRECT) == (
        1, 2, 3, 4, 1)
    assert record.layout_ok()   # ... and laid out as the compiler laid out the built library's
