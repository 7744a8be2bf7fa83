"""What the compiler made of the half-precision DPV reduction kernels (no GPU needed: hipcc cross-compiles): csrc/dpv_half.hip,
read from the code-object metadata of `make dpv_half.s` alone.  Every kernel -- the wave-layout forward in its instantiations
by element type, prob type and planes per lane, the one-pixel-per-thread forward in both summation orders, the backward --:
wave size 64, no spilled register of either kind, no private segment (scratch), workgroups of 256; each wave-layout
instantiation within the registers of its fp32 counterpart, dpv_reduce_ex_vec4_kernel of csrc/dpv.hip."""
import re

from test_isa_guard_dpv import VGPR_LIMIT, _metadata

ELEMS = ("f16_t", "bf16_t")


def _vec4_key(mangled):
    """...dpv_reduce_lp_vec4_kernelINS_5f16_tES2_Li8EE... (prob in the logits' type) | ...INS_6bf16_tEfLi16EE... (prob fp32)
    -> (element type, prob is half, planes per lane)."""
    m = re.search(r"dpv_reduce_lp_vec4_kernelINS_\d+(b?f16_t)E(S\d*_|f)Li(\d+)EE", mangled)
    assert m, mangled
    return m.group(1), m.group(2) != "f", int(m.group(3))


def test_dpv_half_kernels_no_spills_no_scratch_and_keep_their_waves():
    ks = _metadata("dpv_half")
    vec = [n for n in ks if "dpv_reduce_lp_vec4_kernel" in n]
    pixel = [n for n in ks if "dpv_reduce_lp_pixel_kernel" in n]
    bwd = [n for n in ks if "dpv_reduce_lp_bwd_kernel" in n]
    # 2 element types x 2 prob types x (3 planes per lane | 2 summation orders | the backward)
    assert (len(vec), len(pixel), len(bwd)) == (12, 8, 4) and len(ks) == 24, sorted(ks)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256, (name, md)
    assert sorted(_vec4_key(n) for n in vec) == sorted((e, p, r) for e in ELEMS for p in (False, True) for r in (8, 16, 32))
    for name in vec:
        limit = VGPR_LIMIT[("dpv_reduce_ex_vec4_kernel", _vec4_key(name)[2])]
        assert ks[name]["vgpr_count"] + ks[name]["agpr_count"] <= limit, (name, ks[name]["vgpr_count"], limit)
