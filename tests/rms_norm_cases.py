"""The class matrix of the RMS norm kernels (csrc/norm_kernels.inc: rms_norm_fwd_kernel / rms_norm_bwd_kernel), in the style of
tests/norm_class_cases.py: one literal table of calls, each with the kernel class it is MEANT to reach.
tests/test_rms_norm_gpu.py runs every row on the GPU against fp64; tests/test_rms_norm_host.py feeds the same rows to the
compiled csrc/norm_dispatch.h on the CPU and checks that each lands in its labelled class and that the labels cover all five.

Layout shared by both (that of norm_class_cases): every tensor of a call lives alone in a sentinel-filled allocation (256-byte
aligned), PAD elements from its start -- plus one element when its role is listed in ``mis``.

Class labels: "<narrow|wide>/<vec-one|vec-max|scalar>"; "refused": the call must fail with "exceeds" and write nothing."""

PAD = 64
K_MAX_NORM_BLOCKS = 2048                # norm_kernels.inc: the grid cap; 4 waves per workgroup
MANY_ROWS = 4 * K_MAX_NORM_BLOCKS + 3   # 8195: the smallest count at which some wave surely walks two rows
DTYPES = {"16": ("bfloat16", "float16"), "32": ("float32",)}
VEC = {"16": 8, "32": 4}

# roles of each launcher, in the order norm_dispatch.h takes them
ROLES = {"rms_fwd": ("x", "w", "y"), "rms_bwd": ("dy", "x", "w", "dx")}

NV1, NVM, NS, WVM, WS = "narrow/vec-one", "narrow/vec-max", "narrow/scalar", "wide/vec-max", "wide/scalar"
REF = "refused"


def rms(dt, dim, fwd, bwd=None, rows=33, mis=(), null_rstd=False):
    return dict(dt=dt, dim=dim, fwd=fwd, bwd=bwd or fwd, rows=rows, mis=tuple(mis), null_rstd=null_rstd)


RMS_CASES = [
    # ---- 16-bit, V = 8: vector width at its borders
    rms("16", 512, NV1), rms("16", 520, NVM), rms("16", 1024, NVM), rms("16", 1032, WVM), rms("16", 4096, WVM),
    # scalar width forced by dim itself
    rms("16", 37, NS), rms("16", 513, WS), rms("16", 2047, WS),
    # scalar width forced by one misaligned pointer, each role in turn (512: last narrow, 520: first wide, 2048: last)
    rms("16", 512, NS, NS, mis=("x",)), rms("16", 520, WS, WS, mis=("w",)), rms("16", 2048, WS, WVM, mis=("y",)),
    rms("16", 520, NVM, WS, mis=("dy",)), rms("16", 2048, WVM, WS, mis=("dx",)),
    # rows: 1; 3 (a wave of the workgroup has no row); a wave that walks two rows
    rms("16", 64, NV1, rows=1), rms("16", 520, NVM, rows=3), rms("16", 1032, WVM, rows=3), rms("16", 520, WS, WS, rows=3, mis=("x",)),
    rms("16", 64, NV1, rows=MANY_ROWS), rms("16", 37, NS, rows=MANY_ROWS),
    # rstd not asked for
    rms("16", 520, NVM, null_rstd=True), rms("16", 520, WS, NVM, null_rstd=True, mis=("y",)),
    # past the wide limit of each width
    rms("16", 4104, REF), rms("16", 2056, REF, REF, mis=("x",)), rms("16", 2049, REF),
    # ---- fp32, V = 4
    rms("32", 256, NV1), rms("32", 260, NVM), rms("32", 1024, NVM), rms("32", 1028, WVM), rms("32", 4096, WVM),
    rms("32", 37, NS), rms("32", 513, WS), rms("32", 2047, WS),
    rms("32", 512, NS, NS, mis=("w",)), rms("32", 516, WS, WS, mis=("x",)), rms("32", 2048, WS, WVM, mis=("y",)),
    rms("32", 516, NVM, WS, mis=("dy",)), rms("32", 516, NVM, WS, mis=("dx",)),
    rms("32", 64, NV1, rows=1), rms("32", 260, NVM, rows=3), rms("32", 516, WS, WS, rows=3, mis=("x",)),
    rms("32", 64, NV1, rows=MANY_ROWS), rms("32", 37, NS, rows=MANY_ROWS),
    rms("32", 260, NVM, null_rstd=True),
    rms("32", 4100, REF), rms("32", 2052, REF, REF, mis=("x",)), rms("32", 2049, REF),
]


def case_id(c):
    bits = ["rms", c["dt"], str(c["dim"]), f"r{c['rows']}"]
    if c["mis"]:
        bits.append("mis-" + "-".join(c["mis"]))
    if c["null_rstd"]:
        bits.append("null_rstd")
    return "-".join(bits)


def offset(c, role):
    """elements between the start of a role's allocation and its first element"""
    return PAD + (1 if role in c["mis"] else 0)


# what the labels must cover, forward and backward, per dtype group (wide/vec-one cannot exist: a one-chunk row fits the
# narrow instance)
REQUIRED = {NV1, NVM, NS, WVM, WS}
