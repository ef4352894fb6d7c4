"""Registers of the row-wise e4m3 projection's kernels, read from the built library's resource notes the way
tests/test_kernel_resources.py does (its reader, nothing else); no GPU.

The fused kernel is designed for TWO waves per SIMD (one workgroup of 8 waves per CU, as the 16-bit kernel): 512 registers
per SIMD lane / 2 = 256, accumulation registers included.  Its prologue holds a row's 128 registers of 16-bit words while
the 64 of codes appear, so nothing may live in scratch there.  The quantizer keeps a row chunk of 64 fp32 values per lane
between the amax and the conversion: at most 128 registers, 4 waves per SIMD, which hide its two global accesses."""

import test_kernel_resources as KR


def test_fp8_projection_kernels_have_no_scratch_and_fit_their_occupancy():
    ks = KR._kernels()
    fused = {k: v for k, v in ks.items() if "hstu_lnl_fp8_fwd_kernel" in k}
    quant = {k: v for k, v in ks.items() if "hstu_quantize_rows_fp8_kernel" in k}
    assert len(fused) == 2 * 2 and len(quant) == 3, (sorted(fused), sorted(quant))     # I/O dtypes x (LayerNorm or not); source dtypes
    for name, v in {**fused, **quant}.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
    for name, v in fused.items():
        assert v["vgpr"] <= 256, (name, v)        # two waves per SIMD
        assert "hstu_ln_linear_fwd_kernel" not in name
    for name, v in quant.items():
        assert v["vgpr"] <= 128 and v["lds"] == 0, (name, v)        # four waves per SIMD
