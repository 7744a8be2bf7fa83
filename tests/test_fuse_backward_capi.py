"""CPU suite: the C ABI of the DPV fusion backward (pdepth_dpv_fuse_backward_f32) is exported, keeps ABI 6 and validates its
arguments before any launch (no GPU needed: every call below returns before touching a pointer)."""
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native

SYM = "pdepth_dpv_fuse_backward_f32"
FAKE = 256   # a non-null "device pointer": validation fails before any use of it


def _call(logp=FAKE, dmaps=FAKE * 2, masks=FAKE * 3, dc=FAKE * 4, g_f=FAKE * 5, g_l=FAKE * 6, B=1, D=4, H=2, W=2, var=0.3,
          eps=1e-7, out=FAKE * 7):
    lib = _native.load()
    rc = lib.pdepth_dpv_fuse_backward_f32(logp, dmaps, masks, dc, g_f, g_l, B, D, H, W, var, eps, out, None)
    return rc, lib.pdepth_last_error().decode()


def test_symbol_exported_abi_unchanged():
    lib = _native.load()
    assert SYM in _native.EXPORTED_SYMBOLS and hasattr(lib, SYM)
    assert lib.pdepth_abi_version() == 6


@pytest.mark.parametrize("name", ["logp", "dmaps", "masks", "dc", "out"])
def test_null_pointer(name):
    rc, msg = _call(**{name: None})
    assert rc == 1 and msg == SYM + ": null pointer"


def test_no_incoming_gradient():
    rc, msg = _call(g_f=None, g_l=None)
    assert rc == 1 and msg == SYM + ": no incoming gradient"
    # one gradient alone is a valid request: the next check is what answers
    for kw in (dict(g_f=None), dict(g_l=None)):
        rc, msg = _call(D=0, **kw)
        assert rc == 1 and "non-positive dimension" in msg


@pytest.mark.parametrize("dim", ["B", "D", "H", "W"])
@pytest.mark.parametrize("value", [0, -3])
def test_non_positive_dimension(dim, value):
    rc, msg = _call(**{dim: value})
    assert rc == 1 and msg == SYM + ": non-positive dimension"


def test_launch_limits():
    rc, msg = _call(H=1 << 16, W=(1 << 14) + 1)
    assert rc == 1 and "H*W must be at most 2^30" in msg
    rc, msg = _call(B=65536)
    assert rc == 1 and "B at most 65535" in msg
    # the forward entry puts B into grid.y as well and refuses alike, before any launch
    lib = _native.load()
    for kw, what in ((dict(B=65536), "B at most 65535"), (dict(H=1 << 16, W=(1 << 14) + 1), "H*W must be at most 2^30")):
        a = dict(B=1, H=2, W=2)
        a.update(kw)
        rc = lib.pdepth_dpv_fuse_f32(FAKE, FAKE * 2, FAKE * 3, FAKE * 4, a["B"], 4, a["H"], a["W"], 0.3, 1e-7, FAKE * 5, FAKE * 6, None)
        msg = lib.pdepth_last_error().decode()
        assert rc == 1 and msg.startswith("pdepth_dpv_fuse_f32: ") and what in msg


@pytest.mark.parametrize("var", [0.0, -0.3, float("nan")])
def test_var_must_be_positive(var):
    rc, msg = _call(var=var)
    assert rc == 1 and msg == SYM + ": var must be positive"


def test_output_may_not_alias_an_input():
    for kw in (dict(out=FAKE), dict(out=FAKE * 5), dict(out=FAKE * 6)):
        rc, msg = _call(**kw)
        assert rc == 1 and "alias" in msg


def test_binding_checks_shapes_before_the_device():
    x = torch.zeros(1, 6, 4, 4)
    with pytest.raises(RuntimeError, match="no incoming gradient"):
        _native.dpv_fuse_backward(x, torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(6), 0.3, 1e-7)
    with pytest.raises(RuntimeError, match=r"dmaps/masks must be \[B,H,W\] and d_candi \[D\]"):
        _native.dpv_fuse_backward(x, torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(8), 0.3, 1e-7, g_fused=x)
    with pytest.raises(RuntimeError, match="g_logfused must be"):
        _native.dpv_fuse_backward(x, torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(6), 0.3, 1e-7,
                                  g_logfused=torch.zeros(1, 6, 4, 3))
