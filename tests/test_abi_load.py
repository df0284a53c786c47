"""CPU: the C-ABI libraries load and export every symbol include/*.h declares (no compute calls)."""
import ctypes
import os

from conftest import REPO


def _declared(header):
    from spatiotemporalentropymodel_amd import _abi
    return sorted(_abi.prototypes(os.path.join(REPO, "include", header)))


def test_hip_library_exports_header_symbols():
    from spatiotemporalentropymodel_amd import _lib
    names = _declared("stem_hip.h")
    assert len(names) > 30
    lib = ctypes.CDLL(_lib.HIP_SO)
    for n in names:
        assert hasattr(lib, n), f"libstem_hip.so does not export {n}"
    assert set(names) == set(_lib.declared_hip_symbols()), set(names) ^ set(_lib.declared_hip_symbols())
    assert _lib.hip().stem_abi_version() == 5


def test_rans_library_exports_header_symbols():
    from spatiotemporalentropymodel_amd import _lib
    names = _declared("stem_rans.h")
    lib = ctypes.CDLL(_lib.RANS_SO)
    for n in names:
        assert hasattr(lib, n), f"libstem_rans.so does not export {n}"
    assert set(names) == set(_lib.declared_rans_symbols())


def test_dp_library_exports_header_symbols():
    """libstem_dp.so (native RCCL issue path of a data-parallel rank) loads without a GPU and exports what include/stem_dp.h declares"""
    from spatiotemporalentropymodel_amd import _lib
    names = _declared("stem_dp.h")
    assert len(names) == 11
    lib = ctypes.CDLL(_lib.DP_SO)
    for n in names:
        assert hasattr(lib, n), f"libstem_dp.so does not export {n}"
    assert set(names) == set(_lib.declared_dp_symbols())
    d = _lib.dp()
    assert d.stem_dp_submit(None, None, 0, None, 0) != 0 and b"stem_dp_submit" in d.stem_dp_last_error()      # argument checks need no device
    assert d.stem_dp_connect(None, None, 1, 0) != 0 and d.stem_dp_nranks(None) < 0 and d.stem_dp_abort(None, -1, None) != 0


def test_dp_prepare_fails_cleanly_without_a_device():
    """stem_dp_prepare is the LOCAL half of the construction: on a box without a GPU it returns an error with a message and leaves
    the handle NULL -- which is what lets the ranks agree (distributed._NativeIssuer) before any of them enters ncclCommInitRank"""
    import pytest
    import torch
    from spatiotemporalentropymodel_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    d = _lib.dp()
    h = ctypes.c_void_p(1234)
    assert d.stem_dp_prepare(ctypes.byref(h), 0) != 0
    assert not h.value and b"stem_dp_prepare" in d.stem_dp_last_error()


def test_ops_fail_loudly_without_gpu():
    """The product path must not fall back to CPU: CPU tensors are rejected."""
    import pytest
    import torch
    from spatiotemporalentropymodel_amd import functional as F
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    with pytest.raises(RuntimeError):
        F.to_nhwc(torch.zeros(1, 4, 2, 2))


def test_shipped_library_has_no_result_changing_switches():
    """The contract of libstem_hip.so is fp32-class products everywhere: no ablated / instrumented kernel variant and no
    product-count switch exists at all.  The shipped binary does not contain the switches' names, and its plan selectors go
    through stem_tuning_set (validated, no environment)."""
    from spatiotemporalentropymodel_amd import _lib
    lib = _lib.hip()
    blob = open(_lib.HIP_SO, "rb").read()
    for name in (b"STEM_BF16_PRODUCTS", b"STEM_GA_BF16_PRODUCTS", b"STEM_BF16_PRODUCTS_DYN", b"STEM_IGEMM_EXPER", b"STEM_FX3_EXPER",
                 b"STEM_FX3_SPLIT", b"STEM_WG3_SPLIT", b"stem_exper_", b"STEM_EXPERIMENTS",
                 b"STEM_IGEMM_CFG", b"STEM_IGEMM_FUSE_CFG", b"STEM_IGEMM_SPLIT", b"STEM_WGRAD_CFG"):
        assert name not in blob, name
    assert lib.stem_tuning_get(b"fx3_split") == 0 and lib.stem_tuning_get(b"no_such") == -1
    assert lib.stem_tuning_set(b"fx3_split", 3) == 0 and lib.stem_tuning_get(b"fx3_split") == 3
    assert lib.stem_tuning_set(b"fx3_split", 0) == 0
    assert lib.stem_tuning_set(b"fx3_tile", 96) != 0 and b"fx3_tile" in lib.stem_last_error()
    assert lib.stem_tuning_set(b"products", 4) != 0
    # the fp32-MFMA family's plan selectors: round trip, validated with the selector named in the error
    for name, good, bad in ((b"igemm_cfg", (1, 6), (7,)), (b"igemm_fuse_cfg", (2, 5), (1, 3, 4, 6)), (b"igemm_split", (1, 3, 64), ()),
                            (b"wgrad_cfg", (1, 5), (6,))):
        assert lib.stem_tuning_get(name) == 0, name
        for v in good:
            assert lib.stem_tuning_set(name, v) == 0 and lib.stem_tuning_get(name) == v, (name, v)
        for v in bad + (-1,):
            assert lib.stem_tuning_set(name, v) != 0 and lib.stem_tuning_get(name) == good[-1], (name, v)
            assert v < 0 or name in lib.stem_last_error(), (name, v, lib.stem_last_error())
        assert lib.stem_tuning_set(name, 0) == 0 and lib.stem_tuning_get(name) == 0
    # the plan that ran (test aids): readable (0 until the family's first launch in this process), never settable
    for name in (b"igemm_ran_cfg", b"igemm_ran_split", b"wgrad_ran_cfg", b"fx3_ran_form", b"fx3_ran_split", b"fx3_ran_mfma",
                 b"wg3_ran_form", b"wg3_ran_taps", b"wg3_ran_split", b"fx3_col_ran_tile", b"fx3_col_ran_depth", b"fx3_col_ran_mfma",
                 b"tconv_ran_tile", b"tconv_ran_cps", b"tconv_ran_split0", b"tconv_ran_split1", b"tconv_ran_split2", b"tconv_ran_split3"):
        before = lib.stem_tuning_get(name)
        assert before >= 0, name
        assert lib.stem_tuning_set(name, before + 1) != 0 and name in lib.stem_last_error() and b"get-only" in lib.stem_last_error()
        assert lib.stem_tuning_set(name, 0) != 0 and lib.stem_tuning_get(name) == before
