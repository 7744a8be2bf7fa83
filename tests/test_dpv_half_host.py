"""CPU suite: the half-precision entries of the DPV reductions (pdepth_dpv_reduce_ex_lp, pdepth_dpv_reduce_backward_lp) are
declared, bound and exported, and refuse bad arguments before any launch."""
import os
import re

import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdepth_dpv_reduce_ex_lp", "pdepth_dpv_reduce_backward_lp")


def _header():
    return open(os.path.join(REPO, "include", "pdepth.h")).read()


def test_header_binding_and_library_have_the_two_entries():
    h = _header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _native.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        # the binding passes as many arguments as the header declares
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_native._SIGNATURES[name][1]), name
    assert re.search(r"PDEPTH_DTYPE_F16 = (\d+)", h).group(1) == str(_native.DTYPE_F16) == "1"
    assert re.search(r"PDEPTH_DTYPE_BF16 = (\d+)", h).group(1) == str(_native.DTYPE_BF16) == "2"
    assert lib.pdepth_abi_version() == 6 and "#define PDEPTH_ABI_VERSION 6" in h
    mk = open(os.path.join(REPO, "probabilistic-depth_amd", "csrc", "Makefile")).read()
    assert "dpv_half.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()


def test_header_says_what_is_widened_and_what_cannot_alias():
    h = " ".join(_header().split())
    for needed in ("widened to fp32 where it is loaded", "every sum is the fp32 one", "cannot alias the half-precision logits",
                   "rounded to nearest-even"):
        assert needed in h, needed


@pytest.mark.parametrize("dtype", [0, 3])
def test_unknown_dtype_is_refused(dtype):
    lib = _native.load()
    rc = lib.pdepth_dpv_reduce_ex_lp(dtype, 256, None, 256, 1, 4, 4, 4, 256, None, 0, None, None, None, None)
    assert rc == 1 and b"dtype" in lib.pdepth_last_error()
    rc = lib.pdepth_dpv_reduce_backward_lp(dtype, 256, 256, 1, 4, 4, 4, 256, None, 0, None, 512, None)
    assert rc == 1 and b"dtype" in lib.pdepth_last_error()


def test_null_input_no_output_and_the_quarter_rule_are_refused():
    lib = _native.load()
    for dt in (_native.DTYPE_F16, _native.DTYPE_BF16):
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, None, None, 256, 1, 4, 4, 4, 256, None, 0, None, None, None, None)
        assert rc == 1 and b"null input" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, 256, None, None, 1, 4, 4, 4, 256, None, 0, None, None, None, None)
        assert rc == 1 and b"null input" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, 256, None, 256, 1, 4, 4, 4, None, None, 0, None, None, None, None)
        assert rc == 1 and b"no output requested" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, 256, None, 256, 1, 4, 3, 8, 512, None, 0, None, None, 1024, None)
        assert rc == 1 and b"quarter output needs H, W >= 4" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, 256, None, 256, 1, 0, 4, 4, 512, None, 0, None, None, None, None)
        assert rc == 1 and b"non-positive" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_ex_lp(dt, 256, None, 256, 1, 4, 4, 4, 256, None, 0, None, None, None, None)
        assert rc == 1 and b"alias" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_backward_lp(dt, None, 256, 1, 4, 4, 4, 256, None, 0, None, 512, None)
        assert rc == 1 and b"null pointer" in lib.pdepth_last_error()
        rc = lib.pdepth_dpv_reduce_backward_lp(dt, 256, 256, 1, 4, 4, 4, None, None, 0, None, 512, None)
        assert rc == 1 and b"no incoming gradient" in lib.pdepth_last_error()


def test_half_logits_on_the_cpu_still_have_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dpv_reduce(torch.zeros(1, 4, 2, 2, dtype=torch.bfloat16), None, want_depth=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dpv_reduce_ex(torch.zeros(1, 4, 2, 2, dtype=torch.float16), None)
