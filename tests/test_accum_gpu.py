"""Gradient accumulation on an MI355X: k_grad_accum + the ACC forms of the fused engine's optimiser pass
(csrc/optimizer.hip) against the exact fp32 emulation ``utils/schedule.accumulate_reference`` followed by
``clip_reference`` and ``sgd_reference`` / ``adam_reference`` -- every micro-step of eager windows, K = 1, graph replay
with windows that straddle the chunks and the graphs, a new K between two replays, resume in mid-window, two ranks on
one GPU --, the flat ops kernel behind ``grad_accum_``, and the entry points with resume.

Engine cases: the set-up of tests/test_clip_gpu.py, 256 synthetic images, batch 8 (the pass's size is the fixed
76,140-float buffer).  The accumulation buffer is compared bit for bit; the update that follows a window against the
float64 oracles at test_clip_gpu.py's bounds: per tensor (a) state <= 1e-6 relative L2, (b) the increment p' - p <= 1e-4
relative L2; the norm <= 1e-10 relative."""
import functools
import json
import os
import re
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist

from _ranks import spawn_ranks
from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TABLE = [2e-3, 4e-3, 6e-3, 3e-3]
SGD_TABLE = [0.01, 0.02, 0.03, 0.015]
BETAS = (0.9, 0.999)
MU, SGD_WD = 0.9, 5e-4
NDATA, B = 256, 8
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}
# case -> (kind, weight decay, EMA decay, clipping)
CASES = {"sgd": ("sgd", SGD_WD, None, False), "adamw-ema": ("adamw", 5e-2, 0.3, True)}
EPS = 1e-8
TOL, TOL_DELTA, TOL_NORM = 1e-6, 1e-4, 1e-10
OFF_RS = 76076
OFF = 1e30  # a limit no gradient reaches: coef == 1
K = 3


def _opt(case, max_norm, k):
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    kind, wd, ema, _ = CASES[case]
    extra = {} if ema is None else dict(ema_decay=ema, ema_warmup=True)
    if k is not None:
        extra["accumulate_steps"] = k
    if kind == "sgd":
        return OptimizerConfig(momentum=MU, weight_decay=wd, lr_table=SGD_TABLE, max_grad_norm=max_norm, **extra)
    return OptimizerConfig(kind=kind, weight_decay=wd, eps=EPS, betas=BETAS, lr_table=TABLE, max_grad_norm=max_norm,
                           **extra)


def _table(case):
    return SGD_TABLE if CASES[case][0] == "sgd" else TABLE


def _engine(dtype, persistent, optimizer, seed=11, **kw):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    dev = torch.device("cuda", 0)
    data, labels = synthetic_cifar(NDATA, seed=3)
    torch.manual_seed(seed)
    model = NetResDeep().to(dev)
    eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                           EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, optimizer=optimizer, **kw))
    eng.set_indices(list(range(NDATA)))
    eng.set_cursor(0)
    eng.read_loss(reset=True)
    return model, eng


def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def _snap(eng):
    eng.sync()
    torch.cuda.synchronize()
    return dict(params=_cpu(eng.flat), grads=_cpu(eng.grads), m=_cpu(eng.momentum), v=_cpu(eng.exp_avg_sq),
                ema=_cpu(eng.ema), accum=_cpu(eng.accum), gn=None if eng.clip_part is None else eng.grad_norm(),
                step=eng.optimizer_step(), phase=None if eng.accum is None else eng.accumulate_phase(),
                rm=_cpu(eng.bn.running_mean), rv=_cpu(eng.bn.running_var), loss=eng.read_loss()[0])


def _bits(t):
    return t.numpy().tobytes()


def _same(a, b, keys=("params", "m", "v", "ema", "accum", "grads", "rm", "rv"), scalars=("step", "phase", "gn", "loss")):
    for key in keys:
        if a[key] is None:
            assert b[key] is None, key
        else:
            assert _bits(a[key]) == _bits(b[key]), key
    for key in scalars:
        assert a[key] == b[key], (key, a[key], b[key])


def _slices(flat):
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    return [flat[off:off + int(np.prod(shape))] for off, shape in LAYOUT.values()]


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def _clipped(g, coef, inv_ws=1.0):
    """x' = fp32(fp32(g * inv_ws) * coef) of an fp32 gradient slice, as float64."""
    x = (g.double().numpy() * inv_ws).astype(np.float32)
    return (x * np.float32(coef)).astype(np.float32).astype(np.float64)


def _emulate(acc, g, micro, k):
    """One micro-step of k_grad_accum in numpy fp32 over the parameter range."""
    g = g[:OFF_RS].numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        a = g.copy() if micro == 0 else (acc + g).astype(np.float32)
        if micro == k - 1:
            a = (a * (np.float32(1.0) / np.float32(k))).astype(np.float32)
    return a


def _check_update(prev, cur, window, t, lr, case, max_norm, k, inv_ws=1.0, tag=""):
    """cur = the SGD / Adam oracle of (prev state, accumulate_reference(window), t), clipped first where the case
    clips; the EMA follows the new parameters."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at, ema_reference
    from distributeddataparallel_cifar10_amd.utils.schedule import (accumulate_reference, adam_reference, clip_reference,
                                                                  sgd_reference)
    kind, wd, ema, _ = CASES[case]
    g32, _ = accumulate_reference([g[:OFF_RS] for g in window], k)
    assert g32.tobytes() == _bits(cur["accum"][:OFF_RS]), tag
    G = torch.from_numpy(g32)
    coef = np.float32(1.0)
    if max_norm is not None:
        norm, coef = clip_reference(_slices(G), max_norm, inv_ws)
        got_norm = cur["gn"][0]
        print(f"{tag}: norm {got_norm!r} (float64 {norm!r}), coef {float(coef)!r}")
        assert norm > 0 and abs(got_norm - norm) <= TOL_NORM * norm, (tag, got_norm, norm)
    worst, worst_d = 0.0, 0.0
    for name, (off, shape) in LAYOUT.items():
        sl = slice(off, off + int(np.prod(shape)))
        p0 = prev["params"][sl].double().numpy()
        x = _clipped(G[sl], coef, inv_ws)
        if kind == "sgd":
            want = sgd_reference(p0, x, prev["m"][sl], lr, MU, wd)
            keys = ("params", "m")
        else:
            want = adam_reference(p0, x, prev["m"][sl], prev["v"][sl], t, lr, BETAS[0], BETAS[1], EPS, wd,
                                  kind == "adamw")
            keys = ("params", "m", "v")
        got = [cur[key][sl].double().numpy() for key in keys]
        errs = [_rel(g, w) for g, w in zip(got, want)]
        d_want = want[0] - p0
        d_err = _rel(got[0] - p0, d_want)
        worst, worst_d = max(worst, *errs), max(worst_d, d_err)
        for what, err in zip(keys, errs):
            assert err <= TOL, (tag, name, what, err)
        assert d_err <= TOL_DELTA, (tag, name, "increment", d_err)
        assert float(np.abs(d_want).sum()) > 0, (tag, name, "no update")
        if ema is not None:
            err = _rel(cur["ema"][sl].double().numpy(),
                       ema_reference(prev["ema"][sl], cur["params"][sl], ema_decay_at(t - 1, ema, True)))
            assert err <= TOL, (tag, name, "ema", err)
    print(f"{tag}: worst relative L2 (a) {worst:.3e}, (b) {worst_d:.3e}")
    return bool(coef < 1)


@functools.lru_cache(maxsize=None)
def _free_norm(kind, case):
    """The smallest gradient norm of the same run with a limit that is never reached (two optimiser steps)."""
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(case, OFF, K))
    norms = []
    for i in range(7):
        eng.run(B, 1, graph=False)
        if i % K == K - 1:
            norms.append(eng.grad_norm()[0])
    eng.close()
    assert len(norms) == 2 and min(norms) > 0
    return min(norms)


# ---- eager windows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(ENGINES))
def test_eager_windows(gpu, kind, case):
    """K = 3, 7 micro-steps (two windows and one micro-step of a third).  After every micro-step the buffer holds the
    emulation's bits and the latest gradient's CC4 tail; inside a window nothing but the running statistics moves; the
    window's last micro-step is the oracle's update on the accumulated gradient, at the table's entry for the
    optimiser step.  The buffer is poisoned with NaN between the windows: the next one starts from an overwrite."""
    dtype, persistent = ENGINES[kind]
    max_norm = 0.25 * _free_norm(kind, case) if CASES[case][3] else None
    _, eng = _engine(dtype, persistent, _opt(case, max_norm, K))
    assert eng.kind_name == ("sliced" if persistent else "multikernel")
    assert eng.accum is not None and eng.accumulate_phase() == 0 and eng.cfg.optimizer.accumulate_steps == K
    prev = _snap(eng)
    acc, window, flags = None, [], []
    for i in range(7):
        micro = i % K
        eng.run(B, 1, graph=False)
        cur = _snap(eng)
        tag = f"{kind} {case} micro-step {i}"
        acc = _emulate(acc, cur["grads"], micro, K)
        window.append(cur["grads"])
        assert float(cur["grads"][:OFF_RS].abs().sum()) > 0 and not torch.equal(cur["grads"], prev["grads"]), tag
        assert acc.tobytes() == _bits(cur["accum"][:OFF_RS]), tag
        assert _bits(cur["accum"][OFF_RS:OFF_RS + 64]) == _bits(cur["grads"][OFF_RS:OFF_RS + 64]), tag
        assert not torch.isnan(cur["accum"][:OFF_RS + 64]).any(), tag
        assert cur["phase"] == (micro + 1) % K, (tag, cur["phase"])
        assert not torch.equal(cur["rm"], prev["rm"]) and not torch.equal(cur["rv"], prev["rv"]), tag
        if micro < K - 1:  # inside the window: no parameter, no state, no EMA, no counter, no readout moves
            _same(prev, cur, keys=("params", "m", "v", "ema"), scalars=("step", "gn"))
        else:
            t = i // K + 1
            assert cur["step"] == prev["step"] + 1 == t, (tag, cur["step"])
            flags.append(_check_update(prev, cur, window, t, _table(case)[t - 1], case, max_norm, K, tag=tag))
            if max_norm is not None:
                assert cur["gn"][1] == sum(flags), (tag, cur["gn"], flags)
            window = []
            eng.accum.fill_(float("nan"))
            torch.cuda.synchronize()
        prev = cur
    if max_norm is not None:
        assert flags[0], "0.25 x the unclipped norm: the first window's update must clip"
    eng.check_errors()
    eng.close()


@pytest.mark.parametrize("kind", list(ENGINES))
def test_k1_is_off(gpu, kind):
    """accumulate_steps=1: no buffer, and 4 steps bitwise those of the same OptimizerConfig without the field."""
    dtype, persistent = ENGINES[kind]
    out = []
    for k in (None, 1):
        _, eng = _engine(dtype, persistent, _opt("adamw-ema", 0.05, k))
        assert eng.accum is None
        with pytest.raises(RuntimeError, match="accumulation"):
            eng.accumulate_phase()
        eng.run(B, 2, graph=True)
        eng.run(B, 2, graph=False)
        out.append(_snap(eng))
        assert "accum" not in eng.optimizer_state()
        eng.close()
    _same(out[0], out[1])
    assert out[0]["step"] == 4


# ---- graph replay ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ENGINES))
def test_graph_replay_equals_eager_steps(gpu, kind):
    """K = 3, two replays of 16 steps: windows straddle the 8-step chunks and the boundary between the replays (the
    captured graphs do not depend on the phase).  Then set_accumulate_steps(2) between two replays of the captured
    graph: bitwise an eager engine given the same call."""
    dtype, persistent = ENGINES[kind]
    max_norm = 0.25 * _free_norm(kind, "adamw-ema")

    def run(graph):
        _, eng = _engine(dtype, persistent, _opt("adamw-ema", max_norm, K))
        for _ in range(2):
            if graph:
                eng.run(B, 16, graph=True)
            else:
                for _ in range(16):
                    eng.run(B, 1, graph=False)
        first = _snap(eng)
        eng.set_accumulate_steps(2)
        assert eng.accumulate_phase() == 0 and eng.cfg.optimizer.accumulate_steps == 2
        eng.set_cursor(0)
        if graph:
            eng.run(B, 16, graph=True)
        else:
            for _ in range(16):
                eng.run(B, 1, graph=False)
        second = _snap(eng)
        eng.check_errors()
        eng.close()
        return first, second
    g1, g2 = run(True)
    e1, e2 = run(False)
    _same(g1, e1)
    assert g1["step"] == 32 // K and g1["phase"] == 32 % K and g1["gn"][1] >= 1
    _same(g2, e2)
    assert g2["step"] == 32 // K + 8 and g2["phase"] == 0
    assert not torch.equal(g2["params"], g1["params"])


# ---- resume in mid-window ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ENGINES))
def test_resume_in_mid_window(gpu, kind):
    """optimizer_state() taken at phase 2 of 3 (5 micro-steps), loaded with step_state() into a fresh engine: the next
    4 micro-steps (the window's last one, then a whole window) are bitwise the uninterrupted engine's."""
    dtype, persistent = ENGINES[kind]
    max_norm = 0.25 * _free_norm(kind, "adamw-ema")
    model_a, a = _engine(dtype, persistent, _opt("adamw-ema", max_norm, K))
    for _ in range(5):
        a.run(B, 1, graph=False)
    a.sync()
    state = a.optimizer_state()
    assert state["micro"] == 2 and state["step"] == 1 and state["accumulate_steps"] == K
    assert sorted(state) == ["accum", "accumulate_steps", "exp_avg", "exp_avg_sq", "kind", "micro", "step"]
    saved = {key: ({n: t.detach().cpu().clone() for n, t in val.items()} if isinstance(val, dict) else val)
             for key, val in state.items()}
    weights = {n: t.detach().cpu().clone() for n, t in model_a.state_dict().items()}
    ema = {n: t.detach().cpu().clone() for n, t in a.ema_state_dict().items()}
    carried = a.step_state()

    model_b, b = _engine(dtype, persistent, _opt("adamw-ema", max_norm, K), seed=99)
    model_b.load_state_dict(weights)
    b.derive()
    b.load_ema_state_dict(ema)
    b.accum.fill_(float("nan"))
    with pytest.raises(ValueError, match="accumulate_steps"):
        b.load_optimizer_state({**saved, "accumulate_steps": 2})
    with pytest.raises(ValueError, match="micro"):
        b.load_optimizer_state({**saved, "micro": 3})
    b.load_optimizer_state(saved)
    b.load_step_state(carried)
    b.set_cursor(5 * B)
    assert b.accumulate_phase() == 2 and b.optimizer_step() == 1
    for eng in (a, b):
        eng.read_loss(reset=True)
        for _ in range(4):
            eng.run(B, 1, graph=False)
    sa, sb = _snap(a), _snap(b)
    _same(sa, sb, keys=("params", "m", "v", "ema", "grads", "rm", "rv"), scalars=("step", "phase", "loss"))
    assert sa["gn"][0] == sb["gn"][0] > 0  # (the clipped count is a readout since the engine's start, not state)
    assert _bits(sa["accum"][:OFF_RS + 64]) == _bits(sb["accum"][:OFF_RS + 64])
    assert sa["step"] == 3 and sa["phase"] == 0
    a.close()
    b.close()


# ---- two ranks sharing one GPU --------------------------------------------------------------------------------
def _rank_worker(rank, ws, port, dtype, persistent, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["DCA_XGMI_TIMEOUT_S"] = "30"  # a protocol bug ends as an error flag, not a hang
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.data.sampler import distributed_indices
        from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.ddp import FusedDDPTrainer, broadcast_module_state
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        data, labels = synthetic_cifar(NDATA, seed=5)
        order = distributed_indices(NDATA, ws, rank)
        torch.manual_seed(100 + rank)
        model = NetResDeep()
        broadcast_module_state(model, 0)
        model = model.to(dev)
        k = 2
        tr = FusedDDPTrainer(model, data.to(dev), labels.to(dev), batch_max=B, dtype=dtype, persistent=persistent,
                             comm="xgmi", max_indices=len(order), optimizer=_opt("adamw-ema", OFF, k))
        assert tr.comm == "xgmi", tr.comm
        eng = tr.engine
        eng.set_indices(order)
        eng.set_cursor(0)
        eng.read_loss(reset=True)
        prev, window = _snap(eng), []
        for i in range(4):
            eng.run(B, 1)  # graph-captured: step, reduction, all-reduce (sum only), k_grad_accum, norm kernel, the pass
            cur = _snap(eng)
            window.append(cur["grads"])  # the gradient summed over the ranks
            for key in ("params", "m", "v", "ema", "grads"):
                mine = cur[key][:OFF_RS] if key == "ema" else cur[key]  # (the EMA's tail averages the rank's own statistics)
                other = mine.clone()
                dist.broadcast(other, 0)
                assert torch.equal(mine, other), (key, i)
            # CC4 on every micro-step: the running statistics every rank's next step starts from (the RS_BASE region)
            # are rank 0's, as the all-reduced tail carries them -- the same on both ranks.  (A rank's own
            # running_mean / running_var are its step's and differ between the ranks until then, as without
            # accumulation.)
            base = eng.region("RS_BASE", 64).cpu()
            rank0 = torch.cat([cur["rm"], cur["rv"]])
            dist.broadcast(rank0, 0)
            assert _bits(base) == _bits(rank0) == _bits(cur["grads"][OFF_RS:OFF_RS + 64]), i
            assert _bits(cur["accum"][OFF_RS:OFF_RS + 64]) == _bits(cur["grads"][OFF_RS:OFF_RS + 64])
            assert not torch.equal(cur["rm"], prev["rm"]), i
            if i % k < k - 1:
                _same(prev, cur, keys=("params", "m", "v", "ema"), scalars=("step", "gn"))
                assert cur["step"] == prev["step"] and cur["gn"] == prev["gn"]
            else:
                t = i // k + 1
                _check_update(prev, cur, window, t, TABLE[t - 1], "adamw-ema", OFF, k, inv_ws=1.0 / ws,
                              tag=f"rank {rank} micro-step {i}")
                assert cur["step"] == t and cur["gn"][1] == 0
                window = []
            prev = cur
        eng.check_errors()
        assert eng.read_loss()[1] == 4
        tr.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("dtype,persistent", [("bf16", True), ("fp32", False)], ids=["sliced", "multikernel"])
def test_two_ranks_one_gpu(gpu, port, dtype, persistent):
    spawn_ranks(_rank_worker, 2, lambda r: (r, 2, port, dtype, persistent))


# ---- the flat kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 76140, 2 ** 20 + 3])
def test_grad_accum_kernel(gpu, n):
    """grad_accum_ on slices that start 1, 2 and 3 floats into a 16-byte aligned buffer (scalar head, float4 body,
    scalar tail; the largest runs the grid-stride loop), its three forms -- first, add, add + scale -- bitwise against
    numpy fp32, with inf / NaN among the values, and guard elements on both sides of the slice untouched."""
    from distributeddataparallel_cifar10_amd.ops.functional import grad_accum_
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(n)
    scale = np.float32(1.0) / np.float32(3.0)
    for start in (1, 2, 3):
        host_a, host_g = torch.randn(n + 9, generator=gen), torch.randn(n + 9, generator=gen)
        sl = slice(start, start + n)
        special = [float("inf"), float("-inf"), float("nan")]
        for j, val in enumerate(special):  # spread over the slice; with n < 3 the first ones
            host_g[start + (j * (n // 3 + 1)) % n] = val
        host_a[start + n - 1] = float("inf")
        for form in ("first", "add", "add+scale", "first+scale"):
            acc, g = host_a.to(dev), host_g.to(dev)
            assert acc.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
            if form.startswith("first"):
                acc[sl] = float("nan")  # whatever the buffer held
            grad_accum_(acc[sl], g[sl], form.startswith("first"), float(scale) if form.endswith("scale") else None)
            with np.errstate(over="ignore", invalid="ignore"):
                want = host_g[sl].numpy().copy() if form.startswith("first") else \
                    (host_a[sl].numpy() + host_g[sl].numpy()).astype(np.float32)
                if form.endswith("scale"):
                    want = (want * scale).astype(np.float32)
            got_a, got_g = acc.cpu(), g.cpu()
            assert _bits(got_a[sl]) == want.tobytes(), (n, start, form)
            want_g = want if form.endswith("scale") else host_g[sl].numpy()
            assert _bits(got_g[sl]) == want_g.tobytes(), (n, start, form)
            for got, host in ((got_a, host_a), (got_g, host_g)):  # the guards
                assert _bits(got[:start]) == _bits(host[:start]), (n, start, form)
                assert _bits(got[start + n:]) == _bits(host[start + n:]), (n, start, form)
    # slices of differently aligned buffers take the scalar path
    a, g = torch.zeros(n + 8, device=dev), torch.arange(n + 8, device=dev, dtype=torch.float32)
    grad_accum_(a[1:1 + n], g[2:2 + n], True)
    assert torch.equal(a[1:1 + n], g[2:2 + n]) and float(a[0]) == 0 and float(a[1 + n:].abs().sum()) == 0
    with pytest.raises(TypeError):
        grad_accum_(a[:n], g[:n].double(), True)
    with pytest.raises(TypeError):
        grad_accum_(a[:n], g[:n + 1], True)


# ---- entry points ----------------------------------------------------------------------------------------------------
FLAGS = ["--synthetic", "512", "--epochs", "2", "--batch-size", "8", "--accumulate-steps", "3", "--optimizer", "adamw",
         "--clip-grad-norm", "1", "--ema-decay", "0.9"]


def _records(path):
    return [x for x in map(json.loads, open(path).read().splitlines()) if "epoch" in x]


@pytest.mark.parametrize("name", ["fused", "ops"])
def test_main_entry_point_with_accumulation(gpu, tmp_path, name):
    """main.py with the flags above: 64 micro-steps per epoch in windows of 3 that straddle the epochs (21 + 21
    optimiser steps, 2 micro-steps dropped); the metrics fields, the mid-window checkpoint's meta and sidecar."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    mj, ck = tmp_path / "m.json", tmp_path / "birds_vs_airplanes.pt"
    r = subprocess.run([sys.executable, "main.py", "--world-size", "1", *FLAGS, "--engine", name, "--port",
                        str(free_port()), "--checkpoint-path", str(ck), "--metrics-json", str(mj)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Epoch 1, Training loss \d", r.stdout), r.stdout
    assert "--accumulate-steps 3" in r.stderr and "last 2 micro-step" in r.stderr, r.stderr[-2000:]
    recs = _records(str(mj))
    assert [x["steps"] for x in recs] == [64, 64] and [x["optimizer_steps"] for x in recs] == [21, 21]
    for x in recs:
        assert x["accumulate_steps"] == 3 and np.isfinite(x["loss"]) and x["grad_norm"] > 0
        assert 0 <= x["clipped_steps"] <= x["optimizer_steps"]
        assert x["engine"] in (("ops",) if name == "ops" else ("sliced", "multikernel"))
    assert json.load(open(str(ck) + ".meta.json")) == {"epoch": 1, "step": 64, "opt_step": 21, "accum_micro": 1}
    side = torch.load(str(ck) + ".optim.pt", weights_only=True)
    assert sorted(side) == sorted(["accum", "accumulate_steps", "exp_avg", "exp_avg_sq", "kind", "step"] +
                                  (["engine"] if name == "fused" else []))
    assert side["accumulate_steps"] == 3 and side["step"] == 21 and len(side["accum"]) == 9
    assert all(torch.isfinite(v).all() for v in side["accum"].values())
    assert float(side["accum"]["fc2.bias"].abs().sum()) > 0  # (AdamW at lr 1e-2 may leave deeper gradients at zero)
    assert os.path.exists(str(ck) + ".ema.pt")


def _main_flow(monkeypatch, tmp, name, engine, **kw):
    """main.py's per-rank flow at world size 1 with FLAGS; returns the final checkpoint's path and the final EMA."""
    from distributeddataparallel_cifar10_amd import backends
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint
    dev = torch.device("cuda", 0)
    cfg = TrainConfig(synthetic=512, epochs=2, batch_size=8, accumulate_steps=3, optimizer="adamw", clip_grad_norm=1.0,
                      ema_decay=0.9, engine=engine, **kw)
    data, labels = load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=dev,
                          sampler="distributed", seed=0, set_epoch=cfg.set_epoch)
    torch.manual_seed(21)
    model = build_model_for_rank(cfg, 0, 1, dev, data, labels, loader)
    made, real = [], backends.step_backend

    def capture(*a, **k):
        made.append(real(*a, **k))
        return made[-1]
    monkeypatch.setattr(backends, "step_backend", capture)
    try:
        try:
            train_loop(model, loader, 0, cfg)
        except RuntimeError as ex:
            if "injected failure" not in str(ex):
                raise
        backend = made[-1]
        ema = {k: v.detach().cpu().clone() for k, v in backend.ema_state().items()}
        final = save_checkpoint(model, os.path.join(tmp, name + "_final.pt"), 0)
        return final, ema, (backend.micro, backend.optimizer_steps)
    finally:
        monkeypatch.setattr(backends, "step_backend", real)
        if hasattr(model, "close"):
            model.close()


@pytest.mark.parametrize("engine", ["fused", "ops"])
def test_resume_in_mid_window_gives_the_same_checkpoint_and_ema(gpu, tmp_path, monkeypatch, engine):
    """Two epochs straight against one epoch + --resume from its checkpoint, which is in mid-window (phase 1 of 3):
    the final checkpoint and the averaged model are bitwise equal."""
    tmp = str(tmp_path)
    a, ema_a, count_a = _main_flow(monkeypatch, tmp, "a", engine, checkpoint=False)
    assert count_a == (2, 21)
    leg = os.path.join(tmp, "b.pt")
    _main_flow(monkeypatch, tmp, "b1", engine, checkpoint_path=leg, fail_at_step=65)  # epoch 1, stopped at step 65
    assert json.load(open(leg + ".meta.json")) == {"epoch": 1, "step": 64, "opt_step": 21, "accum_micro": 1}
    b, ema_b, count_b = _main_flow(monkeypatch, tmp, "b2", engine, resume=leg, checkpoint=False)
    assert count_b == (2, 21)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert list(ema_a) == list(ema_b)
    for k in ema_a:
        assert torch.equal(ema_a[k], ema_b[k]), k
        assert not torch.equal(ema_a[k].float(), sa[k].float()) or "num_batches" in k
