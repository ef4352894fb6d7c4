"""Replicated in-backward row-wise Adagrad in real process groups (ops/embedding.py, modules/dlrm_hstu.py).

One GPU per test box: the ``nccl`` (= RCCL) branch of the exchange runs as a one-rank group, and the order in which several
ranks' lists are merged is exercised over ``gloo`` with both ranks on device 0 (the rehearsal backend of
``data_parallel.init_from_env``).  RCCL with more than one rank is NOT covered here.  The workers are fresh child processes (a
process group is global state the other tests must not see); each has a time limit, a failed or late worker ends the others,
nothing is retried.  At most two processes have the GPU open."""

import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r'''
import datetime, json, os, sys
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import torch.distributed as dist
from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor
from generative_recommenders_amd.ops import embedding as E

RANK, WORLD, BACKEND = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
torch.cuda.set_device(0)
DEV = torch.device("cuda", 0)
dist.init_process_group(BACKEND, rank=RANK, world_size=WORLD, init_method="tcp://127.0.0.1:%(port)s",
                        timeout=datetime.timedelta(seconds=60))
LR, EPS = 0.05, 1e-8
'''

# ---- 1. one-rank nccl group: three features on two tables, five steps, against the same run without the replicated path
WORKER_NCCL = PRELUDE + r'''
def run(replicated):
    torch.manual_seed(5)
    ec = EmbeddingCollection([EmbeddingConfig(500, 64, "item", ["a", "b"]), EmbeddingConfig(300, 64, "user", ["c"])]).to(DEV)
    ec.apply_rowwise_adagrad_in_backward(lr=LR, eps=EPS, replicated=replicated)
    g = torch.Generator().manual_seed(17)
    for step in range(5):
        ids = {"a": torch.randint(0, 40, (70,), generator=g), "b": torch.randint(20, 60, (50,), generator=g),
               "c": torch.randint(0, 300, (30,), generator=g)}
        feats = KeyedJaggedTensor(["a", "b", "c"], torch.cat([ids[k] for k in "abc"]).to(DEV), torch.tensor([70, 50, 30], device=DEV))
        out = ec(feats)
        sum((out[k].values() * torch.randn(ids[k].numel(), 64, generator=g).to(DEV)).sum() for k in "abc").backward()
    torch.cuda.synchronize()
    return ec

assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
a, b = run(False), run(True)
E.assert_fused_tables_in_sync(b)
sa, sb = a.fused_optimizer_state_dict(), b.fused_optimizer_state_dict()
res = {"weights_equal": all(torch.equal(a.embeddings[t].weight, b.embeddings[t].weight) for t in ("item", "user")),
       "state_equal": all(torch.equal(sa[k], sb[k]) for k in sa), "moved": bool((sa["item.momentum1"] > 0).any()),
       "checksums_equal": E.fused_tables_checksum(a) == E.fused_tables_checksum(b)}
print("RESULT " + json.dumps(res))
dist.destroy_process_group()
'''

# ---- 2. world 2 over gloo: different shards from seeds both ranks know, an empty shard, the formula step by step
WORKER_GLOO = PRELUDE + r'''
import embedding_coalesce_ref as CR
ROWS, DIM, STEPS = 200, 64, 3

def shard(step, rank):
    g = torch.Generator().manual_seed(1000 * step + rank)
    n = 0 if (step == 1 and rank == 1) else 90 + 40 * rank + 7 * step
    return torch.randint(0, 60 + 30 * rank, (n,), generator=g), torch.randn(n, DIM, generator=g)

def collection(average):
    torch.manual_seed(5)
    ec = EmbeddingCollection([EmbeddingConfig(ROWS, DIM, "t", ["c"])]).to(DEV)
    ec.apply_rowwise_adagrad_in_backward(lr=LR, eps=EPS, replicated=True, average=average)
    with torch.no_grad():
        ec.fused_optimizer_state_dict()["t.momentum1"].fill_(0.05)
    if RANK == 1:                                   # rank 1 starts from something else: step 0 is the broadcast
        with torch.no_grad():
            ec.embeddings["t"].weight.add_(1.0)
    E.broadcast_fused_tables(ec, src=0)
    return ec

def step(ec, s):
    idx, dout = shard(s, RANK)
    out = ec(KeyedJaggedTensor(["c"], idx.to(DEV), torch.tensor([idx.numel()], device=DEV)))
    out["c"].values().backward(dout.to(DEV))
    torch.cuda.synchronize()
    return ec.embeddings["t"].weight.detach().cpu().numpy().copy(), ec.fused_optimizer_state_dict()["t.momentum1"].cpu().numpy().copy()

ec = collection(True)
E.assert_fused_tables_in_sync(ec)
states = [(ec.embeddings["t"].weight.detach().cpu().numpy().copy(), ec.fused_optimizer_state_dict()["t.momentum1"].cpu().numpy().copy())]
for s in range(STEPS):
    states.append(step(ec, s))
E.assert_fused_tables_in_sync(ec)
summed = collection(False)
w_sum, m_sum = step(summed, 0)
E.assert_fused_tables_in_sync(summed)
res = {"rank": RANK, "checksum": E.fused_tables_checksum(ec)["t"], "worst": 0.0}
if RANK == 0:
    worst = lambda err, tol: float((err[tol > 0] / tol[tol > 0]).max())
    for s in range(STEPS):
        parts = [shard(s, r) for r in range(WORLD)]                 # rank order
        idx, dout = torch.cat([p[0] for p in parts]).numpy(), torch.cat([p[1] for p in parts]).numpy()
        (w0, m0), (w1, m1) = states[s], states[s + 1]
        ref = CR.replicated_adagrad_ref(w0, m0, idx, dout, LR, EPS, 1.0 / WORLD)
        rows = ref["rows"]
        err_w = np.abs(w1[rows].astype(np.float64) - ref["weight"][rows])
        err_m = np.abs(m1[rows].astype(np.float64) - ref["momentum1"][rows])
        res["worst"] = max(res["worst"], worst(err_w, ref["tol_weight"]), worst(err_m, ref["tol_momentum1"]))
        assert (err_w <= ref["tol_weight"]).all() and (err_m <= ref["tol_momentum1"]).all(), f"step {s}"
        keep = np.ones(ROWS, dtype=bool)
        keep[rows] = False
        assert keep.any() and np.array_equal(w1[keep], w0[keep]) and np.array_equal(m1[keep], m0[keep]), f"step {s}: untouched rows"
        if s == 0:                                  # summed instead of averaged: far outside the bound on every touched row
            gap_m = np.abs(m_sum[rows].astype(np.float64) - m1[rows])
            gap_w = np.abs(w_sum[rows].astype(np.float64) - w1[rows])
            assert (gap_m > 100 * ref["tol_momentum1"]).all() and gap_w.max() > 100 * ref["tol_weight"].max()
            res["average_gap_over_bound"] = float((gap_m / ref["tol_momentum1"]).min())
print("RESULT " + json.dumps(res))
dist.barrier()
dist.destroy_process_group()
'''

# ---- 3. the small DlrmHSTU: a GradientAllReducer over model.parameters() next to replicated fused tables
WORKER_DLRM = PRELUDE + r'''
import dlrm_hstu_ref as R
from generative_recommenders_amd import data_parallel as dp
from generative_recommenders_amd.modules.dlrm_hstu import apply_rowwise_adagrad_in_backward

inputs = R.load("model_small")
names = [n for n, _, _ in R.TASKS]
model = R.build(False, inputs).to(DEV)
model.set_training_dtype(torch.float32)
apply_rowwise_adagrad_in_backward(model, lr=LR, eps=EPS, replicated=True)
E.broadcast_fused_tables(model)
red = dp.GradientAllReducer(model.parameters())
dense = torch.optim.SGD([p for n, p in model.named_parameters() if not n.startswith("_embedding_collection.")], lr=1e-3)

def features(step):
    """the fixture's batch with the item ids rotated by an amount that depends on the rank and the step"""
    out = []
    for keys, values, lengths in (("uih_keys", "uih_values", "uih_lengths"), ("candidate_keys", "candidate_values", "candidate_lengths")):
        k = [str(x) for x in inputs[keys]]
        v, l = torch.from_numpy(np.ascontiguousarray(inputs[values])).clone(), torch.from_numpy(np.ascontiguousarray(inputs[lengths]))
        sizes = l.view(len(k), -1).sum(dim=1).tolist()
        o = 0
        for key, size in zip(k, sizes):
            if key in ("uih_item_id", "cand_item_id"):
                v[o:o + size] = (v[o:o + size] + 7 * RANK + 3 * step) %% 50
            o += size
        out.append(KeyedJaggedTensor(k, v.to(DEV), l.to(DEV)))
    return out

before = E.fused_tables_checksum(model)
for s in range(3):
    for p in model.parameters():
        p.grad = None
    out = model(*features(s))
    torch.stack([out[2][n] for n in names]).sum().backward()
    tables = [p for n, p in model.named_parameters() if n.startswith("_embedding_collection.")]
    assert all(p.grad is None for p in tables), "a fused table received a gradient"
    red.reduce()
    assert all(p.grad is None or not bool(p.grad.any()) for p in tables)        # the reducer brings no gradient to them
    dense.step()
torch.cuda.synchronize()
E.assert_fused_tables_in_sync(model)
bits = lambda t: int(t.detach().contiguous().view(torch.int32).sum(dtype=torch.int64))
res = {"rank": RANK, "params": {n: bits(p) for n, p in model.named_parameters()}, "tables": E.fused_tables_checksum(model),
       "tables_moved": E.fused_tables_checksum(model) != before}
print("RESULT " + json.dumps(res))
dist.barrier()
dist.destroy_process_group()
'''


def _run_workers(tmp_path, source, world, backend, limit):
    """start ``world`` workers, wait at most ``limit`` seconds for all of them; the first failure or the deadline ends the rest"""
    script = tmp_path / "worker.py"
    script.write_text(source % {"root": ROOT, "port": str(29700 + os.getpid() % 200)})
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    logs = [open(tmp_path / f"rank{r}.log", "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), backend], stdout=logs[r], stderr=subprocess.STDOUT,
                              env=env, cwd=ROOT) for r in range(world)]
    deadline, failed = time.monotonic() + limit, None
    try:
        while failed is None and any(p.poll() is None for p in procs):
            if time.monotonic() > deadline:
                failed = f"not finished after {limit} s"
            elif any(p.poll() not in (None, 0) for p in procs):
                failed = "a worker failed"
            else:
                try:
                    next(p for p in procs if p.poll() is None).wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    texts = []
    for f in logs:
        f.seek(0)
        texts.append(f.read())
        f.close()
    codes = [p.returncode for p in procs]
    assert failed is None and codes == [0] * world, (failed, codes, [t[-3000:] for t in texts])
    results = []
    for t in texts:
        line = [ln for ln in t.splitlines() if ln.startswith("RESULT ")]
        assert line, t[-2000:]
        results.append(json.loads(line[-1][7:]))
    return results


def test_one_rank_rccl_group_is_bit_identical_to_the_one_shot_path(tmp_path):
    (res,) = _run_workers(tmp_path, WORKER_NCCL, 1, "nccl", 240)
    assert res == {"weights_equal": True, "state_equal": True, "moved": True, "checksums_equal": True}, res


def test_two_ranks_over_gloo_stay_in_sync_and_match_the_formula(tmp_path):
    r0, r1 = sorted(_run_workers(tmp_path, WORKER_GLOO, 2, "gloo", 240), key=lambda r: r["rank"])
    print(f"two ranks over gloo: worst err/bound {r0['worst']:.3f}; summed vs averaged momentum1 gap {r0['average_gap_over_bound']:.3g} x bound")
    assert r0["checksum"] == r1["checksum"]
    assert 0 < r0["worst"] <= 1.0


def test_dlrm_hstu_two_ranks_dense_reducer_and_replicated_tables(tmp_path):
    r0, r1 = sorted(_run_workers(tmp_path, WORKER_DLRM, 2, "gloo", 300), key=lambda r: r["rank"])
    assert r0["tables_moved"] and r1["tables_moved"]
    assert r0["tables"] == r1["tables"] and len(r0["tables"]) == 2
    assert r0["params"] == r1["params"] and len(r0["params"]) > 2
