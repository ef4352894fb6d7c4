"""The class matrix of the row-norm kernels (csrc/norm_ops.hip, norm_kernels.inc): one literal table of calls, each with
the kernel class it is MEANT to reach.  tests/test_norm_classes_gpu.py runs every row on the GPU against fp64;
tests/test_norm_dispatch_host.py feeds the same rows to the compiled csrc/norm_dispatch.h on the CPU and checks that each
lands in its labelled class and that the labels cover every launch line -- a row that is silently routed elsewhere fails
there, without a GPU.

Layout shared by both: every tensor of a call lives alone in a sentinel-filled allocation (256-byte aligned, which is what
torch's allocator hands out), PAD elements from its start -- plus one element when its role is listed in ``mis``.  PAD is
a 16-byte multiple in every dtype, so a role is 16-byte aligned iff it is not in ``mis``.

Class labels
  ln / swish / l2 : "<narrow|wide>/<vec-one|vec-max|scalar>"  (l2 has no one-chunk instantiation: "vec" there)
  nm              : "<narrow|wide>/<gn-fast-one|gn-fast-max|gn-vec|gn-scalar|ln-vec|ln-scalar>/<silu|plain>"
  silu            : "vec" | "scalar"
  "refused"       : the call must fail with "exceeds" and write nothing
"""

PAD = 64
K_MAX_NORM_BLOCKS = 2048            # norm_kernels.inc: the grid cap; 4 waves per workgroup
MANY_ROWS = 4 * K_MAX_NORM_BLOCKS + 3   # 8195: the smallest count at which some wave surely walks two rows
DTYPES = {"16": ("bfloat16", "float16"), "32": ("float32",)}
VEC = {"16": 8, "32": 4}

# roles of each launcher, in the order norm_dispatch.h takes them
ROLES = {
    "ln_fwd": ("x", "w", "b", "y"),
    "ln_bwd": ("dy", "x", "w", "b", "dres", "dx"),          # b: swish only; dres: with the fused residual only
    "nm_fwd": ("attn", "u", "w", "b", "y"),
    "nm_bwd": ("dy", "attn", "u", "w", "b", "dattn", "du"),
    "l2_fwd": ("x", "g", "y"),                              # g absent in the forward
    "l2_bwd": ("x", "dy", "dx"),
    "silu_fwd": ("dout", "in", "out"),                      # dout absent in the forward
    "silu_bwd": ("dout", "in", "din"),
}


def _c(op, dt, fwd, bwd, dim=None, heads=1, hd=None, rows=33, gn=False, mis=(), ustride=0, dustride=0, concat=False,
       silu=False, drop=0.0, res=False, null_stats=False, name=None):
    if dim is None:
        dim = heads * hd
    if hd is None:
        hd = dim // heads
    assert heads * hd == dim
    return dict(op=op, dt=dt, fwd=fwd, bwd=bwd, dim=dim, heads=heads, hd=hd, rows=rows, gn=gn, mis=tuple(mis),
                ustride=ustride or dim, dustride=dustride or dim, concat=concat, silu=silu, drop=drop, res=res,
                null_stats=null_stats, name=name)


def ln(dt, dim, fwd, bwd=None, **kw):
    return _c("ln", dt, fwd, bwd or fwd, dim=dim, **kw)


def swish(dt, dim, fwd, bwd=None, **kw):
    return _c("swish", dt, fwd, bwd or fwd, dim=dim, **kw)


def l2(dt, dim, fwd, bwd=None, **kw):
    return _c("l2", dt, fwd, bwd or fwd, dim=dim, **kw)


def nm(dt, heads, hd, cls, bwd=None, silu=False, **kw):
    s = "/silu" if silu else "/plain"
    lab = lambda k: k if k == REF else k + s
    return _c("nm", dt, lab(cls), lab(bwd or cls), heads=heads, hd=hd, silu=silu, **kw)


def silu(dt, cols, fwd, bwd=None, **kw):
    """cols wide column slice: ustride = row stride of the input, dustride = of the output (default: cols)"""
    return _c("silu", dt, fwd, bwd or fwd, dim=cols, **kw)


NV1, NVM, NS, WVM, WS = "narrow/vec-one", "narrow/vec-max", "narrow/scalar", "wide/vec-max", "wide/scalar"
REF = "refused"

# ------------------------------------------------------------------------------------------------ layer norm (+ residual)
LN_CASES = [
    # ---- 16-bit, V = 8: vector width at its borders
    ln("16", 512, NV1), ln("16", 520, NVM), ln("16", 1024, NVM), ln("16", 1032, WVM), ln("16", 4096, WVM),
    # scalar width forced by dim itself
    ln("16", 37, NS), ln("16", 513, WS), ln("16", 2047, WS),
    # scalar width forced by one misaligned pointer, each role in turn (512: last narrow, 520: first wide, 2048: last)
    ln("16", 512, NS, NS, mis=("x",)), ln("16", 520, WS, WS, mis=("w",)), ln("16", 520, WS, NVM, mis=("b",)),
    ln("16", 2048, WS, WVM, mis=("y",)), ln("16", 520, NVM, WS, mis=("dy",)), ln("16", 2048, WVM, WS, mis=("dx",)),
    ln("16", 800, WS, NVM, mis=("b",), name="ln_fwd_dim800_bias_misaligned"),
    ln("16", 800, WS, WS, mis=("w",), name="ln_bwd_dim800_weight_misaligned"),
    # the fused residual: every class, and the residual pointer as the spoiler
    ln("16", 512, NV1, res=True), ln("16", 1024, NVM, res=True), ln("16", 1032, WVM, res=True), ln("16", 37, NS, res=True),
    ln("16", 520, NVM, WS, res=True, mis=("dres",)), ln("16", 800, NVM, WS, res=True, mis=("dres",), name="ln_bwd_dim800_dresidual_misaligned"),
    ln("16", 2047, WS, res=True),
    # rows: 1; 3 (a wave of the workgroup has no row); a wave that walks two rows
    ln("16", 64, NV1, rows=1), ln("16", 520, NVM, rows=3), ln("16", 1032, WVM, rows=3), ln("16", 520, WS, WS, rows=3, mis=("x",)),
    ln("16", 64, NV1, rows=MANY_ROWS), ln("16", 37, NS, rows=MANY_ROWS, res=True),
    # mean / rstd not asked for
    ln("16", 520, NVM, null_stats=True), ln("16", 520, WS, NVM, null_stats=True, mis=("y",)),
    # past the wide limit of each width
    ln("16", 4104, REF), ln("16", 2056, REF, REF, mis=("x",)), ln("16", 2049, REF), ln("16", 4104, REF, res=True),
    # ---- fp32, V = 4
    ln("32", 256, NV1), ln("32", 260, NVM), ln("32", 1024, NVM), ln("32", 1028, WVM), ln("32", 4096, WVM),
    ln("32", 37, NS), ln("32", 513, WS), ln("32", 2047, WS),
    ln("32", 512, NS, NS, mis=("w",)), ln("32", 516, WS, WS, mis=("x",)), ln("32", 516, WS, NVM, mis=("b",)),
    ln("32", 2048, WS, WVM, mis=("y",)), ln("32", 516, NVM, WS, mis=("dy",)), ln("32", 516, NVM, WS, mis=("dx",)),
    ln("32", 800, WS, NVM, mis=("b",), name="ln_fwd_dim800_bias_misaligned_fp32"),
    ln("32", 256, NV1, res=True), ln("32", 260, NVM, res=True), ln("32", 1028, WVM, res=True), ln("32", 513, WS, res=True), ln("32", 37, NS, res=True),
    ln("32", 516, NVM, WS, res=True, mis=("dres",)),
    ln("32", 64, NV1, rows=1), ln("32", 260, NVM, rows=3), ln("32", 516, WS, WS, rows=3, mis=("x",)),
    ln("32", 64, NV1, rows=MANY_ROWS), ln("32", 37, NS, rows=MANY_ROWS),
    ln("32", 260, NVM, null_stats=True),
    ln("32", 4100, REF), ln("32", 2052, REF, REF, mis=("x",)), ln("32", 2049, REF), ln("32", 4100, REF, res=True),
]

# ------------------------------------------------------------------------------------------------ swish layer norm
SWISH_CASES = [
    swish("16", 512, NV1), swish("16", 520, NVM), swish("16", 1032, WVM), swish("16", 4096, WVM),
    swish("16", 37, NS), swish("16", 513, WS), swish("16", 2047, WS),
    swish("16", 512, NS, NS, mis=("x",)), swish("16", 520, WS, WS, mis=("w",)), swish("16", 520, WS, WS, mis=("b",)),
    swish("16", 520, WS, NVM, mis=("y",)), swish("16", 520, NVM, WS, mis=("dy",)), swish("16", 2048, WVM, WS, mis=("dx",)),
    swish("16", 520, NVM, rows=3), swish("16", 37, NS, rows=MANY_ROWS), swish("16", 520, NVM, null_stats=True),
    swish("16", 4104, REF), swish("16", 2056, REF, REF, mis=("b",)),
    swish("32", 256, NV1), swish("32", 260, NVM), swish("32", 1028, WVM), swish("32", 4096, WVM),
    swish("32", 37, NS), swish("32", 513, WS), swish("32", 2047, WS),
    swish("32", 512, NS, NS, mis=("b",)), swish("32", 516, WS, WS, mis=("x",)), swish("32", 516, WS, NVM, mis=("y",)),
    swish("32", 2048, WVM, WS, mis=("dx",)),
    swish("32", 260, NVM, rows=3), swish("32", 64, NV1, rows=MANY_ROWS),
    swish("32", 4100, REF), swish("32", 2052, REF, REF, mis=("w",)),
]

# ------------------------------------------------------------------------------------------------ u * Norm(attn)
# every launch line of nm_fwd / nm_bwd in the narrow and the wide instance, each with SiLU on and off; concat, dropout and
# the u / du strides are spread over them so that every kernel sees concat on and off and dropout on and off
N, W = "narrow/", "wide/"
CAT_DROP = dict(concat=True, drop=0.25)
NM_CASES = [
    # ---- 16-bit: layer norm, vector
    nm("16", 4, 128, N + "ln-vec", **CAT_DROP), nm("16", 4, 128, N + "ln-vec", silu=True),
    nm("16", 5, 104, N + "ln-vec", concat=True), nm("16", 8, 128, N + "ln-vec", silu=True, drop=0.25),
    nm("16", 8, 128, N + "ln-vec", silu=True, ustride=3 * 1024, dustride=3 * 1024, **CAT_DROP),   # u / du in place in a uvqk-shaped buffer
    nm("16", 3, 344, W + "ln-vec", **CAT_DROP), nm("16", 3, 344, W + "ln-vec", silu=True),
    nm("16", 16, 256, W + "ln-vec", silu=True, concat=True), nm("16", 16, 256, W + "ln-vec", drop=0.25),
    # layer norm, scalar: by dim, and by every fact in turn
    nm("16", 1, 37, N + "ln-scalar", **CAT_DROP), nm("16", 1, 37, N + "ln-scalar", silu=True),
    nm("16", 4, 128, N + "ln-scalar", mis=("attn",), silu=True, **CAT_DROP), nm("16", 4, 128, N + "ln-scalar", mis=("u",)),
    nm("16", 1, 513, W + "ln-scalar", silu=True, **CAT_DROP), nm("16", 23, 89, W + "ln-scalar"),
    nm("16", 5, 104, W + "ln-scalar", mis=("attn",)), nm("16", 5, 104, W + "ln-scalar", mis=("u",), silu=True, concat=True),
    nm("16", 5, 104, W + "ln-scalar", mis=("w",), drop=0.25), nm("16", 5, 104, W + "ln-scalar", mis=("b",), silu=True),
    nm("16", 5, 104, W + "ln-scalar", N + "ln-vec", mis=("y",), concat=True),
    nm("16", 5, 104, N + "ln-vec", W + "ln-scalar", mis=("dy",), silu=True, **CAT_DROP),
    nm("16", 5, 104, N + "ln-vec", W + "ln-scalar", mis=("dattn",)), nm("16", 5, 104, N + "ln-vec", W + "ln-scalar", mis=("du",), silu=True),
    nm("16", 5, 104, W + "ln-scalar", ustride=524, silu=True), nm("16", 5, 104, N + "ln-vec", W + "ln-scalar", dustride=524, concat=True),
    nm("16", 8, 100, W + "ln-scalar", ustride=804, silu=True, name="nm_fwd_ln_dim800_u_stride_804"),
    nm("16", 8, 100, N + "ln-vec", W + "ln-scalar", dustride=804, silu=True, name="nm_bwd_ln_dim800_du_stride_804"),
    nm("16", 16, 128, W + "ln-scalar", mis=("attn",), **CAT_DROP), nm("16", 16, 128, W + "ln-scalar", ustride=2052, dustride=2052, silu=True),
    # group norm, fast path: one chunk, several chunks narrow and wide
    nm("16", 4, 128, N + "gn-fast-one", gn=True, **CAT_DROP), nm("16", 4, 128, N + "gn-fast-one", gn=True, silu=True),
    nm("16", 3, 64, N + "gn-fast-one", gn=True, silu=True, ustride=4 * 192, dustride=4 * 192, **CAT_DROP),
    nm("16", 2, 256, N + "gn-fast-one", gn=True, drop=0.25),
    nm("16", 9, 64, N + "gn-fast-max", gn=True, **CAT_DROP), nm("16", 8, 128, N + "gn-fast-max", gn=True, silu=True),
    nm("16", 16, 64, N + "gn-fast-max", gn=True, silu=True, **CAT_DROP), nm("16", 2, 512, N + "gn-fast-max", gn=True),
    nm("16", 9, 128, W + "gn-fast-max", gn=True, **CAT_DROP), nm("16", 16, 256, W + "gn-fast-max", gn=True, silu=True),
    nm("16", 16, 128, W + "gn-fast-max", gn=True, silu=True, **CAT_DROP), nm("16", 5, 256, W + "gn-fast-max", gn=True, drop=0.25),
    # group norm, generic vector path (lanes per head not a power of two)
    nm("16", 3, 40, N + "gn-vec", gn=True, **CAT_DROP), nm("16", 8, 96, N + "gn-vec", gn=True, silu=True),
    nm("16", 8, 96, N + "gn-vec", gn=True, silu=True, **CAT_DROP), nm("16", 13, 40, N + "gn-vec", gn=True),
    nm("16", 13, 80, W + "gn-vec", gn=True, **CAT_DROP), nm("16", 16, 96, W + "gn-vec", gn=True, silu=True),
    nm("16", 16, 240, W + "gn-vec", gn=True, silu=True, concat=True), nm("16", 16, 96, W + "gn-vec", gn=True, drop=0.25),
    # group norm, scalar: head_dim % 8, a pointer, a stride
    nm("16", 4, 100, N + "gn-scalar", gn=True, **CAT_DROP), nm("16", 3, 37, N + "gn-scalar", gn=True, silu=True),
    nm("16", 4, 128, N + "gn-scalar", gn=True, mis=("attn",), silu=True, concat=True),
    nm("16", 8, 100, W + "gn-scalar", gn=True, name="nm_fwd_gn_8x100"), nm("16", 8, 100, W + "gn-scalar", gn=True, silu=True, **CAT_DROP),
    nm("16", 5, 104, W + "gn-scalar", gn=True, mis=("u",), silu=True), nm("16", 5, 104, W + "gn-scalar", N + "gn-vec", gn=True, mis=("y",), drop=0.25),
    nm("16", 5, 104, N + "gn-vec", W + "gn-scalar", gn=True, mis=("dy",), concat=True),
    nm("16", 5, 104, N + "gn-vec", W + "gn-scalar", gn=True, mis=("dattn",), silu=True),
    nm("16", 5, 104, N + "gn-vec", W + "gn-scalar", gn=True, mis=("du",)),
    nm("16", 5, 104, W + "gn-scalar", gn=True, ustride=524), nm("16", 5, 104, N + "gn-vec", W + "gn-scalar", gn=True, dustride=524, silu=True),
    nm("16", 16, 128, W + "gn-scalar", gn=True, mis=("attn",), silu=True, **CAT_DROP),
    # weight / bias misaligned with group norm: read as scalars per head, so the class stays a vector one
    nm("16", 4, 128, N + "gn-fast-one", gn=True, mis=("w", "b")),
    # rows
    nm("16", 2, 32, N + "gn-fast-one", gn=True, rows=1, silu=True, **CAT_DROP), nm("16", 1, 64, N + "ln-vec", rows=1),
    nm("16", 9, 64, N + "gn-fast-max", gn=True, rows=3, **CAT_DROP), nm("16", 5, 104, N + "ln-vec", rows=3, silu=True),
    nm("16", 8, 100, W + "gn-scalar", gn=True, rows=3, silu=True), nm("16", 5, 104, W + "ln-scalar", rows=3, mis=("u",), **CAT_DROP),
    nm("16", 2, 32, N + "gn-fast-one", gn=True, rows=MANY_ROWS, **CAT_DROP), nm("16", 1, 64, N + "ln-vec", rows=MANY_ROWS, silu=True),
    nm("16", 3, 21, N + "gn-scalar", gn=True, rows=MANY_ROWS, silu=True), nm("16", 1, 37, N + "ln-scalar", rows=MANY_ROWS, concat=True),
    # refusals: the wide limit + 1 at each width; more than 16 heads with group norm
    nm("16", 1, 4104, REF), nm("16", 1, 2056, REF, mis=("u",)), nm("16", 8, 257, REF, gn=True), nm("16", 1, 2049, REF),
    # ---- fp32, V = 4
    nm("32", 2, 128, N + "ln-vec", **CAT_DROP), nm("32", 5, 52, N + "ln-vec", silu=True),
    nm("32", 4, 256, N + "ln-vec", silu=True, ustride=3 * 1024, dustride=3 * 1024, **CAT_DROP), nm("32", 8, 128, N + "ln-vec", drop=0.25),
    nm("32", 4, 257, W + "ln-vec", **CAT_DROP), nm("32", 16, 256, W + "ln-vec", silu=True),
    nm("32", 1, 37, N + "ln-scalar", silu=True, **CAT_DROP), nm("32", 4, 128, N + "ln-scalar", mis=("attn",)),
    nm("32", 1, 513, W + "ln-scalar", **CAT_DROP), nm("32", 4, 129, W + "ln-scalar", mis=("w",), silu=True),
    nm("32", 4, 129, W + "ln-scalar", mis=("u",)), nm("32", 4, 129, W + "ln-scalar", mis=("b",), silu=True, concat=True),
    nm("32", 4, 129, W + "ln-scalar", N + "ln-vec", mis=("y",)), nm("32", 4, 129, N + "ln-vec", W + "ln-scalar", mis=("dy",), silu=True),
    nm("32", 4, 129, N + "ln-vec", W + "ln-scalar", mis=("dattn",), **CAT_DROP), nm("32", 4, 129, N + "ln-vec", W + "ln-scalar", mis=("du",)),
    nm("32", 8, 100, W + "ln-scalar", ustride=802, silu=True, name="nm_fwd_ln_dim800_u_stride_802_fp32"),
    nm("32", 8, 100, N + "ln-vec", W + "ln-scalar", dustride=801, name="nm_bwd_ln_dim800_du_stride_801_fp32"),
    nm("32", 16, 128, W + "ln-scalar", mis=("attn",), silu=True, **CAT_DROP),
    nm("32", 4, 64, N + "gn-fast-one", gn=True, **CAT_DROP), nm("32", 2, 128, N + "gn-fast-one", gn=True, silu=True),
    nm("32", 8, 64, N + "gn-fast-max", gn=True, silu=True, **CAT_DROP), nm("32", 5, 64, N + "gn-fast-max", gn=True),
    nm("32", 9, 128, W + "gn-fast-max", gn=True, **CAT_DROP), nm("32", 16, 256, W + "gn-fast-max", gn=True, silu=True),
    nm("32", 3, 40, N + "gn-vec", gn=True, silu=True, **CAT_DROP), nm("32", 8, 96, N + "gn-vec", gn=True),
    nm("32", 13, 80, W + "gn-vec", gn=True, **CAT_DROP), nm("32", 16, 96, W + "gn-vec", gn=True, silu=True),
    nm("32", 4, 102, N + "gn-scalar", gn=True, silu=True, **CAT_DROP), nm("32", 4, 128, N + "gn-scalar", gn=True, mis=("u",)),
    nm("32", 8, 102, W + "gn-scalar", gn=True, name="nm_fwd_gn_8x102_fp32", **CAT_DROP), nm("32", 8, 102, W + "gn-scalar", gn=True, silu=True),
    nm("32", 4, 132, W + "gn-scalar", N + "gn-vec", gn=True, mis=("y",)), nm("32", 4, 132, N + "gn-vec", W + "gn-scalar", gn=True, mis=("du",), silu=True),
    nm("32", 4, 132, W + "gn-scalar", gn=True, ustride=530, concat=True), nm("32", 4, 132, N + "gn-vec", W + "gn-scalar", gn=True, dustride=529),
    nm("32", 2, 32, N + "gn-fast-one", gn=True, rows=1), nm("32", 5, 64, N + "gn-fast-max", gn=True, rows=3, silu=True, **CAT_DROP),
    nm("32", 8, 102, W + "gn-scalar", gn=True, rows=3), nm("32", 5, 52, N + "ln-vec", rows=3, **CAT_DROP),
    nm("32", 2, 32, N + "gn-fast-one", gn=True, rows=MANY_ROWS, silu=True), nm("32", 1, 37, N + "ln-scalar", rows=MANY_ROWS, **CAT_DROP),
    nm("32", 1, 4100, REF), nm("32", 1, 2052, REF, mis=("attn",)), nm("32", 8, 257, REF, gn=True),
]
# (no group-norm row has ONE head: its dweight / dbias is then a single cancelling sum, whose relative error is its condition
# number times the fp32 round-off, and a relative gate on one such number says nothing -- a 1 x 512 row drew sum|t| / |sum t|
# of 4.9e3 (bf16) and 2.0e4 (fp16); numpy's fp32 sum of the same terms is off by 4e-6 and 8e-5 there.  64 lanes per head, the
# most the segmented kernels take, is the 2 x 512 row)
# the 16-head limit of group norm is a refusal of its own (not a class): checked by the GPU test directly
GN_TOO_MANY_HEADS = dict(heads=17, hd=32)

# ------------------------------------------------------------------------------------------------ row L2 norm
NV, WV = "narrow/vec", "wide/vec"
L2_CASES = [
    l2("16", 512, NV), l2("16", 1024, NV), l2("16", 1032, WV), l2("16", 4096, WV),
    l2("16", 37, NS), l2("16", 513, WS), l2("16", 2047, WS),
    l2("16", 512, NS, NS, mis=("x",)), l2("16", 520, WS, NV, mis=("y",)), l2("16", 520, NV, WS, mis=("dy",)),
    l2("16", 2048, WV, WS, mis=("dx",)), l2("16", 2048, WS, WS, mis=("x",)),
    l2("16", 64, NV, rows=1), l2("16", 520, NV, rows=3), l2("16", 64, NV, rows=MANY_ROWS), l2("16", 37, NS, rows=MANY_ROWS),
    l2("16", 4104, REF), l2("16", 2056, REF, REF, mis=("x",)),
    l2("32", 256, NV), l2("32", 1024, NV), l2("32", 1028, WV), l2("32", 4096, WV),
    l2("32", 37, NS), l2("32", 513, WS), l2("32", 2047, WS),
    l2("32", 512, NS, NS, mis=("x",)), l2("32", 516, WS, NV, mis=("y",)), l2("32", 516, NV, WS, mis=("dy",)),
    l2("32", 2048, WV, WS, mis=("dx",)),
    l2("32", 64, NV, rows=1), l2("32", 260, NV, rows=3), l2("32", 37, NS, rows=MANY_ROWS),
    l2("32", 4100, REF), l2("32", 2052, REF, REF, mis=("x",)),
]

# ------------------------------------------------------------------------------------------------ SiLU on a column slice
SILU_CASES = [
    silu("16", 64, "vec"), silu("16", 512, "vec", ustride=1536, dustride=520), silu("16", 4096, "vec"),
    silu("16", 37, "scalar"), silu("16", 64, "scalar", ustride=100), silu("16", 64, "scalar", dustride=68),
    silu("16", 64, "scalar", mis=("in",)), silu("16", 64, "scalar", mis=("out", "din")), silu("16", 64, "vec", "scalar", mis=("dout",)),
    silu("16", 64, "vec", rows=1), silu("16", 37, "scalar", rows=3, ustride=41, dustride=39, mis=("in",)),
    silu("32", 64, "vec"), silu("32", 256, "vec", ustride=768, dustride=260), silu("32", 4096, "vec"),
    silu("32", 37, "scalar"), silu("32", 64, "scalar", ustride=99), silu("32", 64, "scalar", dustride=66),
    silu("32", 64, "scalar", mis=("in",)), silu("32", 64, "scalar", mis=("out", "din")), silu("32", 64, "vec", "scalar", mis=("dout",)),
    silu("32", 37, "scalar", rows=3, ustride=41, dustride=39, mis=("in",)),
]

CASES = LN_CASES + SWISH_CASES + NM_CASES + L2_CASES + SILU_CASES


def case_id(c):
    if c["name"]:
        return c["name"]
    bits = [c["op"], c["dt"], f"{c['heads']}x{c['hd']}" if c["op"] == "nm" else str(c["dim"]), f"r{c['rows']}"]
    if c["gn"]:
        bits.append("gn")
    if c["mis"]:
        bits.append("mis-" + "-".join(c["mis"]))
    if c["ustride"] != c["dim"]:
        bits.append(f"us{c['ustride']}")
    if c["dustride"] != c["dim"]:
        bits.append(f"ds{c['dustride']}")
    for flag in ("concat", "silu", "res", "null_stats"):
        if c[flag]:
            bits.append(flag)
    if c["drop"]:
        bits.append("drop")
    return "-".join(bits)


def offset(c, role):
    """elements between the start of a role's allocation and its first element"""
    return PAD + (1 if role in c["mis"] else 0)


# ---- what the labels must cover: every launch line of every launcher, in every instance that can reach it, per dtype group
_LN_LINES = {NV1, NVM, NS, WVM, WS}          # wide/vec-one cannot exist: a one-chunk row fits the narrow instance
_NM_KERNELS = ("gn-fast-one", "gn-fast-max", "gn-vec", "gn-scalar", "ln-vec", "ln-scalar")
_NM_LINES = {f"{i}{k}/{s}" for i in (N, W) for k in _NM_KERNELS for s in ("silu", "plain")} - {W + "gn-fast-one/silu", W + "gn-fast-one/plain"}
_L2_LINES = {NV, NS, WV, WS}
REQUIRED = {
    ("ln", "fwd"): _LN_LINES, ("ln", "bwd"): _LN_LINES, ("ln+res", "bwd"): _LN_LINES,
    ("swish", "fwd"): _LN_LINES, ("swish", "bwd"): _LN_LINES,
    ("nm", "fwd"): _NM_LINES, ("nm", "bwd"): _NM_LINES,
    ("l2", "fwd"): _L2_LINES, ("l2", "bwd"): _L2_LINES,
    ("silu", "fwd"): {"vec", "scalar"}, ("silu", "bwd"): {"vec", "scalar"},
}
