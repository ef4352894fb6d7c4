"""The int8 quantize and gather kernels keep everything in registers: no scratch, no spills, no LDS.  Reads the resource
notes of the built library the way tests/test_kernel_resources.py does (its reader, nothing else); no GPU."""

import test_kernel_resources as KR


def test_int8_row_kernels_use_no_scratch_and_stay_at_full_occupancy_registers():
    ks = {k: v for k, v in KR._kernels().items() if "rows_int8_kernel" in k}
    quantize = {k: v for k, v in ks.items() if "quantize_rows_int8_kernel" in k}
    gather = {k: v for k, v in ks.items() if "gather_rows_int8_kernel" in k}
    assert len(quantize) == 3 * 2 and len(gather) == 3 * 2 + 2, sorted(ks)       # dtypes x passes; dtypes x index types, + fp32's second pass
    for name, v in ks.items():
        assert v["scratch"] == 0 and v["spill"] == 0 and v["lds"] == 0, (name, v)
        assert v["vgpr"] <= 64, (name, v)                                         # 8 waves per SIMD: the gather lives on loads in flight
