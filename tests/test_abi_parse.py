"""CPU: the header reader behind the ctypes bindings (spatiotemporalentropymodel_amd/_abi.py) -- type classes on synthetic headers,
spot checks on include/*.h, descriptor layouts against the LP64 rules, and every bound function against the parse."""
import ctypes as C
import os

import pytest

from conftest import REPO

from spatiotemporalentropymodel_amd import _abi

SYNTHETIC = """
/* a comment with ; and ( and stem_x( inside; int stem_not_declared(int a); */
#ifndef T_H
#define T_H
#include <stddef.h>
#define STEM_T_LONG_MACRO 8 /* spans
                             * lines; stem_y( */
#ifdef __cplusplus
extern "C" {
#endif
enum { STEM_T_A = 0, STEM_T_B = 1 };  // trailing ; ( stem_z(
typedef struct {
    const float *x;   /* pointer; first */
    int K, C, R;
    long sh, sw;
    void *p;
    unsigned n;
} stem_t_desc;
typedef int (*stem_t_fn)(void *ctx, const int32_t *in, size_t n);
const char *stem_t_error(void);
void *stem_t_create(void);
void stem_t_destroy(void *h);
size_t stem_t_bytes(int a, unsigned b, unsigned int c, long d, unsigned long e, long long f, unsigned long long g);
long stem_t_scalars(float a, double b, size_t c, uint64_t d, int64_t e, int32_t f, uint32_t g, const int h);
int stem_t_wrapped(const float *x, int ldx,
                   void **out, void *const *many, const int32_t *idx /* [n] */,
                   const unsigned char *bytes, uint8_t *raw, const stem_t_desc *descs, const char *name, stem_t_fn cb,
                   const float *const *tensors, unsigned long long *sse, char *writable);
#ifdef __cplusplus
}
#endif
#endif
"""


def _write(tmp_path, text, name="t.h"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_type_classes_on_a_synthetic_header(tmp_path):
    vp = C.c_void_p
    header = _write(tmp_path, SYNTHETIC)
    protos = _abi.prototypes(header)
    assert set(protos) == {"stem_t_error", "stem_t_create", "stem_t_destroy", "stem_t_bytes", "stem_t_scalars", "stem_t_wrapped"}   # nothing out of a comment
    assert protos["stem_t_error"] == (C.c_char_p, [])                      # `(void)`; const char * as a return
    assert protos["stem_t_create"] == (vp, [])
    assert protos["stem_t_destroy"] == (None, [vp])                        # void return
    assert protos["stem_t_bytes"] == (C.c_size_t, [C.c_int, C.c_uint, C.c_uint, C.c_long, C.c_ulong, C.c_longlong, C.c_ulonglong])
    assert protos["stem_t_scalars"] == (C.c_long, [C.c_float, C.c_double, C.c_size_t, C.c_uint64, C.c_int64, C.c_int32, C.c_uint32, C.c_int])
    # wrapped over three lines; every pointer but `const char *` is void *, and so is the callback typedef
    assert protos["stem_t_wrapped"] == (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_char_p, vp, vp, vp, vp])
    assert _abi.structs(header) == {"stem_t_desc": [("x", vp), ("K", C.c_int), ("C", C.c_int), ("R", C.c_int), ("sh", C.c_long), ("sw", C.c_long),
                                                    ("p", vp), ("n", C.c_uint)]}


@pytest.mark.parametrize("decl, names", [
    ("int stem_t_bad(int a, foo_t b);", ("stem_t_bad", "foo_t")),                                   # a type outside the map
    ("int stem_t_bad(const foo_t *b);", ("stem_t_bad", "foo_t")),                                   # ... behind a pointer
    ("foo_t stem_t_bad(int a);", ("stem_t_bad", "foo_t")),                                          # ... as the return
    ("int stem_t_bad(int n, float v[4]);", ("stem_t_bad", "float v[4]")),                           # an array parameter
    ("typedef struct { int a; } stem_t_s;\nint stem_t_bad(stem_t_s s);", ("stem_t_bad", "stem_t_s")),   # an aggregate by value
    ("int stem_t_bad(struct foo s);", ("stem_t_bad", "struct foo")),
    ("int stem_t_bad(int a, int);", ("stem_t_bad", "int")),                                         # half read: no parameter name
    ("int stem_t_bad(int a, int (*cb)(int));", ("stem_t_bad",)),                                    # half read: a declarator in a declarator
    ("int stem_t_bad(int a)\nint stem_t_next(void);", ("stem_t_bad",)),                             # half read: a lost semicolon
    ("int stem_t_bad();", ("stem_t_bad",)),                                                         # neither parameters nor (void)
    ("static const int stem_t_table = 4;", ("stem_t_table",)),                                      # not a function declaration
    ("typedef struct { float v[4]; } stem_t_s;", ("stem_t_s", "float v[4]")),
    ("typedef struct { foo_t a; } stem_t_s;", ("stem_t_s", "foo_t")),
    ("typedef struct { float *a, *b; } stem_t_s;", ("stem_t_s", "float *a, *b")),
])
def test_what_the_reader_cannot_map_raises(tmp_path, decl, names):
    with pytest.raises(_abi.HeaderError) as err:
        _abi.prototypes(_write(tmp_path, "#include <stddef.h>\n" + decl + "\n"))
    for text in names:
        assert text in str(err.value), (text, str(err.value))


def _real(header):
    return _abi.prototypes(os.path.join(REPO, "include", header))


def test_spot_checks_on_the_real_headers():
    vp, hip = C.c_void_p, _real("stem_hip.h")
    assert len(hip) == 146 and len(_real("stem_rans.h")) == 13 and len(_real("stem_dp.h")) == 11
    args = {n: a for n, (_, a) in hip.items()}
    assert len(args["stem_conv2d_fwd"]) == 20 and args["stem_conv2d_fwd"][16] is C.c_float and args["stem_conv2d_fwd"][18] is C.c_size_t
    assert args["stem_wgrad_bias_parts"][4] is C.c_long
    assert args["stem_uniform_noise"][2] is C.c_uint64 and args["stem_uniform_noise"][3] is C.c_uint64
    assert args["stem_em_loss_finalize"][4] is C.c_double
    assert args["stem_tuning_set"] == [C.c_char_p, C.c_int]
    assert args["stem_stream_flag_wait_ge"][1] is C.c_uint
    assert args["stem_stream_flag_create"] == [vp]                                   # void **
    assert len(args["stem_ar_decode_image"]) == 39 and args["stem_ar_decode_image"][31] is vp     # stem_symbol_decoder_fn decode
    assert [i for i, a in enumerate(args["stem_ar_decode_image"]) if a is C.c_float] == [27, 28]
    assert hip["stem_tape_create"][0] is vp
    assert hip["stem_tape_destroy"][0] is None
    assert hip["stem_packed_weight_elems"][0] is C.c_size_t
    assert hip["stem_last_error"][0] is C.c_char_p
    assert _real("stem_rans.h")["stem_rans_encode"][0] is C.c_long
    assert _real("stem_dp.h")["stem_dp_abort"] == (C.c_int, [vp, C.c_int, C.c_char_p])


def test_descriptor_layouts_follow_the_lp64_rules():
    """sizes and offsets worked out by hand from include/stem_hip.h (8-byte pointers and longs, 4-byte ints, natural alignment)"""
    from spatiotemporalentropymodel_amd import _lib
    sizes = {"PackDesc": 40, "UnpackDesc": 40, "BiasFinalDesc": 32, "F16PackDesc": 64, "F16PairDesc": 72, "WaveSeg": 40}
    for name, size in sizes.items():
        cls = getattr(_lib, name)
        assert issubclass(cls, C.Structure) and C.sizeof(cls) == size, (name, C.sizeof(cls))
    assert (_lib.F16PairDesc.wp0.offset, _lib.F16PairDesc.wp1.offset, _lib.F16PairDesc.bmax.offset) == (24, 40, 56)
    assert _lib.F16PackDesc.bmax.offset == 40
    assert _lib.WaveSeg.sh.offset == 16
    assert [f for f, _ in _lib.PackDesc._fields_] == ["w", "wp", "K", "C", "R", "S", "role", "masked"]
    assert len(_abi.structs(os.path.join(REPO, "include", "stem_hip.h"))) == len(sizes)          # every typedef struct has its class


def test_every_bound_function_carries_the_header_prototype():
    """_bind leaves no function at ctypes' implicit defaults (restype int, argtypes unset)"""
    from spatiotemporalentropymodel_amd import _lib
    for lib, header, names in ((_lib.hip(), "stem_hip.h", _lib.declared_hip_symbols()), (_lib.rans(), "stem_rans.h", _lib.declared_rans_symbols()),
                               (_lib.dp(), "stem_dp.h", _lib.declared_dp_symbols())):
        protos = _real(header)
        assert sorted(protos) == names
        for name, (restype, argtypes) in protos.items():
            fn = getattr(lib, name)
            assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
            assert all(a is b for a, b in zip(fn.argtypes, argtypes)), (name, fn.argtypes, argtypes)
            assert fn.restype is restype, (name, fn.restype, restype)
    assert _lib._HIP_SIG == {n: a for n, (_, a) in _real("stem_hip.h").items()}                                # what tape.py classifies slots by
    assert set(_lib._RESTYPE) == {n for n, (r, _) in _real("stem_hip.h").items() if r is not C.c_int}       # what tape.py keeps out of a schedule


def test_a_missing_header_is_named(monkeypatch, tmp_path):
    from spatiotemporalentropymodel_amd import _lib
    monkeypatch.setattr(_lib, "_PKG", str(tmp_path / "pkg"))
    with pytest.raises(_lib.StemLibraryError, match="stem_hip.h"):
        _lib._tables("stem_hip.h")
