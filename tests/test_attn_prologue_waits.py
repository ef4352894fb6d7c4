"""No compiler-placed memory drain in the prologues of the attention kernels the benchmark dispatches (CPU only: the code
objects inside libhstu_hip.so are taken apart as tests/test_kernel_resources.py does).

A `s_waitcnt vmcnt(0)` waits for EVERYTHING the wave has in flight -- in a persistent kernel that is the previous problem's
stores and the tile requests of this one.  The kernels place the ones they need by hand; hipcc used to add three more (a
spill reload in front of a problem's first request, the join of a conditional flat load of attn_scale behind the prologue's
requests, the last Q row of the forward behind the first two tiles' requests: docs/EXPERIMENTS.md R21).  Per kernel:

  * no scratch segment and no spilled register (ELF notes);
  * no flat load (attn_scale goes through the constant address space: a scalar load, counted by lgkmcnt);
  * as many `s_waitcnt vmcnt(0)` as the source writes by hand for that instantiation (table below);
  * forward, head dim 128: nothing reads or writes the Q-row registers between their hand-issued loads and the counted wait that hands them to the compiler (hstu_attn_fwd.cuh, q_rows_issue /
    q_rows_wait: the compiler does not know they are in flight)."""
import os
import re
import subprocess
import tempfile

import pytest

from test_kernel_resources import LIB, OBJDUMP, READELF, _code_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")

# mangled-name fragment -> (hand-written vmcnt(0) waits, where the source writes them)
FOLD_STEP = ("hstu_attn_bwd_fold.cuh", 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', "fold_problem_x: top of every step, in front of its barrier")
QUAD_STEP = ("hstu_attn_bwd_quad.cuh", 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', "quad_problem: top of every step, in front of its barrier")
FWD_LAST = ("hstu_attn_fwd.cuh", 'else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', "tile loop, COUNTED: the last tile has nothing requested behind it")
FWD_CLAMP = ("hstu_attn_fwd.cuh", r"\n\ts_waitcnt vmcnt(0)", "q_rows_load_clamped: head dim below the instantiated one, one overload per KG")
# head dim 64 keeps the compiler's loads of the Q rows (the hand-written wait measured slower there, docs/EXPERIMENTS.md R21): the
# vmcnt(3) .. vmcnt(0) chain behind them is the ONE compiler-placed drain this file accepts
FWD_Q_CHAIN_D64 = (None, None, "compiler-placed: the last of the four Q-row waits, head dim 64 only")
EXPECTED = {
    "hstu_attn_bwd_fold_kernelIDF16bLi128ELi128E": [FOLD_STEP],      # bf16, d = 128
    "hstu_attn_bwd_fold_kernelIDF16_Li128ELi128E": [FOLD_STEP],      # f16
    "hstu_attn_bwd_fold_kernelIDF16bLi64ELi64E": [FOLD_STEP],        # d = 64 (HSTU_BWD_QUAD=0)
    "hstu_attn_bwd_quad_kernelIDF16bLi64E": [QUAD_STEP],             # d = 64
    "hstu_attn_fwd_kernelIDF16bLi128ELi128ELb0ELb0ELb0E": [FWD_LAST, FWD_CLAMP],
    "hstu_attn_fwd_kernelIDF16bLi64ELi64ELb0ELb0ELb0E": [FWD_LAST, FWD_Q_CHAIN_D64],
    "hstu_attn_fwd_kernelIDF16_Li128ELi128ELb0ELb0ELb0E": [FWD_LAST, FWD_CLAMP],
}
# how often each statement stands in its source file (all instantiations together): a new hand-written drain shows up here
SOURCE_COUNT = {FOLD_STEP: 1, QUAD_STEP: 1, FWD_LAST: 1, FWD_CLAMP: 2}


def _tools():
    if not (os.path.exists(LIB) and os.path.exists(READELF) and os.path.exists(OBJDUMP)):
        pytest.skip("library or llvm tools not available")


_CACHE = {}


def _kernels():
    """{mangled name: (notes dict, [instruction lines])} of the kernels named in EXPECTED"""
    if _CACHE:
        return _CACHE
    _tools()
    data = open(LIB, "rb").read()
    for co in _code_objects(data):
        if not any(f.encode() in co for f in EXPECTED):
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        meta = {}
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and any(f in name.group(1) for f in EXPECTED):
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
                meta[name.group(1)] = dict(vgpr=get("vgpr_count"), spill=get("vgpr_spill_count"), scratch=get("private_segment_fixed_size"))
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1) if m.group(1) in meta else None
                if cur:
                    _CACHE[cur] = (meta[cur], [])
            elif cur and line.strip():
                _CACHE[cur][1].append(re.sub(r"\s*//.*$", "", line.strip()))
    return _CACHE


def _one(frag):
    hits = [(k, v) for k, v in _kernels().items() if frag in k]
    assert len(hits) == 1, (frag, [k for k, _ in hits])
    return hits[0]


def test_source_statements_are_where_the_table_says():
    for (fname, text, _), n in SOURCE_COUNT.items():
        src = open(os.path.join(CSRC, fname)).read()
        assert src.count(text) == n, (fname, text, src.count(text))


@pytest.mark.parametrize("frag", sorted(EXPECTED))
def test_no_scratch_no_spill_no_flat_load(frag):
    name, (meta, ins) = _one(frag)
    assert meta["scratch"] == 0 and meta["spill"] == 0, (name, meta)
    flat = [i for i in ins if i.startswith("flat_load")]
    assert not flat, (name, flat)
    assert not [i for i in ins if i.startswith("scratch_")], name


@pytest.mark.parametrize("frag", sorted(EXPECTED))
def test_every_full_drain_is_hand_written(frag):
    name, (_, ins) = _one(frag)
    drains = [i for i in ins if i.startswith("s_waitcnt") and "vmcnt(0)" in i]
    assert len(drains) == len(EXPECTED[frag]), (name, drains, [w[2] for w in EXPECTED[frag]])


def _vregs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}
    return out


@pytest.mark.parametrize("frag,loads_wanted,per_tile,waits", [
    ("hstu_attn_fwd_kernelIDF16bLi128ELi128ELb0ELb0ELb0E", 8, 4, 1),
    ("hstu_attn_fwd_kernelIDF16_Li128ELi128ELb0ELb0ELb0E", 8, 4, 1)])
def test_hand_issued_rows_are_untouched_until_their_wait(frag, loads_wanted, per_tile, waits):
    """q_rows_wait is `vmcnt(2 PER_TILE)`, a branch, `vmcnt(PER_TILE)`; the row loads in front of it share one address register
    pair per tensor.  From the first of them to the last wait no other instruction may name one of their destination registers.
    (With two tensors the first tensor's registers are free from the first wait on; the check keeps them until the second, which
    follows it directly.)"""
    name, (_, ins) = _one(frag)
    w = [i for i in range(len(ins) - 2) if ins[i] == f"s_waitcnt vmcnt({2 * per_tile})" and ins[i + 1].startswith("s_branch")
         and ins[i + 2] == f"s_waitcnt vmcnt({per_tile})"]
    assert len(w) == waits, (name, w)
    loads = []
    for i in range(w[0] - 1, -1, -1):
        m = re.match(r"global_load_dwordx4 (v\[\d+:\d+\]), (v\[\d+:\d+\]), off", ins[i])
        if m and "lds" not in ins[i]:
            loads.append((i, m.group(1), m.group(2)))
            if len(loads) == loads_wanted:
                break
    assert len(loads) == loads_wanted and len({a for _, _, a in loads}) == waits, (name, loads)
    dst_of = {i: (_vregs(dst), _vregs(addr)) for i, dst, addr in loads}
    assert len(set().union(*(d for d, _ in dst_of.values()))) == 4 * loads_wanted
    in_flight, touched = set(), []
    for i in range(min(dst_of), w[-1] + 3):        # in program order: a register is in flight from its load on
        if i in dst_of:
            assert not (dst_of[i][1] & in_flight), (name, "a row load's address lies in a register that is in flight", ins[i])
            in_flight |= dst_of[i][0]
        elif _vregs(ins[i]) & in_flight:
            touched.append(ins[i])
    assert not touched, (name, touched)
