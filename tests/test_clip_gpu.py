"""Global gradient-norm clipping on an MI355X: k_grad_sqnorm + the CLIP forms of the fused engine's optimiser pass
(csrc/optimizer.hip) against the float64 oracle ``utils/schedule.clip_reference`` followed by ``sgd_reference`` /
``adam_reference`` -- the readout, the coef == 1 path, every clipped update, graph replay, a new limit between two
replays, two ranks on one GPU --, the flat ops kernels ``k_sqnorm_part`` / ``k_clip_coef`` and the ``gscale`` forms of
``k_sgd`` / ``k_adam``, and the entry points with resume.

Engine cases: the set-up of tests/test_adam_gpu.py, 256 synthetic images, batch 8 (the pass's size is the fixed
76,140-float buffer).  Bounds:

* the norm <= 1e-10 relative to float64: every (double)x * (double)x is exact and 76,074 double additions err by at
  most n * 2^-53 = 8.4e-12 relative, whatever their order;
* per tensor, as test_adam_gpu.py derives them: (a) state (p', buffer or m', v') <= 1e-6 relative L2, (b) the increment
  p' - p <= 1e-4 relative L2 against the oracle's.  The oracle receives the clipped gradient x' = fp32(fp32(g * inv_ws)
  * coef), so the clipping adds nothing to either but the fp32 rounding of x' itself (6e-8) where the test forms it;
* the norm after clipping, coef * N <= max_norm * (1 + 1e-6): coef <= fp32(max_norm / N), 6e-8 above it at most."""
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
SGD_TABLE = [0.01, 0.02, 0.03, 0.015]  # (tests/test_optimizer_gpu.py's)
BETAS = (0.9, 0.999)
MU, SGD_WD = 0.9, 5e-4
NDATA, B = 256, 8
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}
# case -> (kind, weight decay, EMA decay)
CASES = {"sgd": ("sgd", SGD_WD, None), "adamw": ("adamw", 5e-2, None), "adam-l2": ("adam", 5e-4, None),
         "adamw-ema": ("adamw", 5e-2, 0.3)}
EPS = 1e-8
TOL, TOL_DELTA, TOL_NORM = 1e-6, 1e-4, 1e-10
OFF_RS = 76076
OFF = 1e30  # a limit no gradient reaches: coef == 1


def _opt(case, max_norm):
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    kind, wd, ema = CASES[case]
    extra = {} if ema is None else dict(ema_decay=ema, ema_warmup=True)
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


def _snap(eng):
    eng.sync()
    torch.cuda.synchronize()
    return dict(params=eng.flat.detach().cpu().clone(), grads=eng.grads.detach().cpu().clone(),
                m=eng.momentum.detach().cpu().clone(),
                v=None if eng.exp_avg_sq is None else eng.exp_avg_sq.detach().cpu().clone(),
                ema=None if eng.ema is None else eng.ema.detach().cpu().clone(),
                gn=None if eng.clip_part is None else eng.grad_norm(),
                step=eng.optimizer_step(), loss=eng.read_loss()[0])


@functools.lru_cache(maxsize=None)
def _eager_steps(kind, case, max_norm):
    """Five single eager steps; the state before and after every step.  `max_norm` None: clipping off."""
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(case, max_norm))
    assert eng.kind_name == ("sliced" if persistent else "multikernel")
    assert (eng.clip_part is None) == (max_norm is None)
    snaps = [_snap(eng)]
    for _ in range(5):
        eng.run(B, 1, graph=False)
        snaps.append(_snap(eng))
    eng.check_errors()
    eng.close()
    return snaps


def _limit(kind, case):
    """0.25 x the smallest norm of the run whose limit is never reached."""
    return 0.25 * min(s["gn"][0] for s in _eager_steps(kind, case, OFF)[1:])


def _slices(flat):
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    return [flat[off:off + int(np.prod(shape))] for off, shape in LAYOUT.values()]


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def _clipped(g, coef, inv_ws=1.0):
    """x' = fp32(fp32(g * inv_ws) * coef) of an fp32 gradient slice, as float64."""
    x = (g.double().numpy() * inv_ws).astype(np.float32)
    return (x * np.float32(coef)).astype(np.float32).astype(np.float64)


def _check_step(prev, cur, t, lr, case, max_norm, inv_ws=1.0, tag=""):
    """cur's readout = clip_reference(cur's grads over the LAYOUT slices); cur = the SGD / Adam oracle of (prev state,
    the clipped gradient, t).  Returns whether the step clipped."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.schedule import adam_reference, clip_reference, sgd_reference
    kind, wd, _ = CASES[case]
    norm, coef = clip_reference(_slices(cur["grads"]), max_norm, inv_ws)
    whole = float(np.sqrt(np.sum((cur["grads"][:OFF_RS + 64].double().numpy() * inv_ws) ** 2)))
    got_norm = cur["gn"][0]
    print(f"{tag}: norm {got_norm!r} (float64 {norm!r}, with the CC4 tail {whole!r}), coef {float(coef)!r}")
    assert norm > 0 and abs(got_norm - norm) <= TOL_NORM * norm, (tag, got_norm, norm)
    if inv_ws != 1.0:  # several ranks: the CC4 tail holds the summed running statistics, which the norm must leave out
        assert abs(whole - norm) > 1e-6 * norm, (tag, "the tail is too small for this check to see it", whole, norm)
    assert float(coef) * norm <= max_norm * (1 + 1e-6), (tag, coef, norm, max_norm)
    worst, worst_d, least = 0.0, 0.0, np.inf
    for name, (off, shape) in LAYOUT.items():
        sl = slice(off, off + int(np.prod(shape)))
        p0 = prev["params"][sl].double().numpy()
        x = _clipped(cur["grads"][sl], coef, inv_ws)
        if kind == "sgd":
            want = sgd_reference(p0, x, prev["m"][sl], lr, MU, wd)
            keys = ("params", "m")
        else:
            want = adam_reference(p0, x, prev["m"][sl], prev["v"][sl], t, lr, BETAS[0], BETAS[1], EPS, wd,
                                  kind == "adamw")
            keys = ("params", "m", "v")
        got = [cur[k][sl].double().numpy() for k in keys]
        errs = [_rel(g, w) for g, w in zip(got, want)]
        d_want = want[0] - p0
        rms = float(np.sqrt(np.mean(d_want ** 2)))
        d_err = _rel(got[0] - p0, d_want)
        worst, worst_d, least = max(worst, *errs), max(worst_d, d_err), min(least, rms / lr)
        for what, err in zip(keys, errs):
            assert err <= TOL, (tag, name, what, err)
        assert d_err <= TOL_DELTA, (tag, name, "increment", d_err, rms / lr)
        assert float(cur["grads"][sl].abs().sum()) > 0, (tag, name, "no gradient")
    print(f"{tag}: worst relative L2 (a) {worst:.3e}, (b) {worst_d:.3e}; least rms(increment) / lr {least:.3e}")
    return bool(coef < 1)


# ---- the readout and the coef == 1 path -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(ENGINES))
def test_readout_and_unit_coefficient(gpu, kind, case):
    """max_grad_norm = 1e30: every step's grad_norm() is the float64 norm of that snapshot's gradient over the LAYOUT
    slices (not the CC4 tail, not the pads), no step counts as clipped, and the run is bitwise the one without
    clipping."""
    from distributeddataparallel_cifar10_amd.utils.schedule import clip_reference
    on, off = _eager_steps(kind, case, OFF), _eager_steps(kind, case, None)
    assert on[0]["gn"] == (0.0, 0) and off[0]["gn"] is None
    for k in range(1, 6):
        norm, coef = clip_reference(_slices(on[k]["grads"]), OFF)
        got, clipped = on[k]["gn"]
        print(f"{kind} {case} step {k - 1}: norm {got!r}, float64 {norm!r}")
        assert coef == np.float32(1.0) and clipped == 0
        assert norm > 0 and abs(got - norm) <= TOL_NORM * norm, (k, got, norm)
    for k in range(6):
        for key in ("params", "m", "v", "ema", "grads"):
            if on[k][key] is None:
                assert off[k][key] is None
            else:
                assert torch.equal(on[k][key], off[k][key]), (k, key)
        assert on[k]["loss"] == off[k]["loss"] and on[k]["step"] == off[k]["step"] == k


# ---- clipping ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(ENGINES))
def test_clipped_update_matches_reference(gpu, kind, case):
    """max_norm = 0.25 x the smallest norm of the unclipped run: step 0 sees the same gradient in both runs, so it
    clips; every step against clip_reference + the SGD / Adam oracle from its own snapshot."""
    max_norm = _limit(kind, case)
    snaps, free = _eager_steps(kind, case, max_norm), _eager_steps(kind, case, OFF)
    assert torch.equal(snaps[1]["grads"], free[1]["grads"]) and snaps[1]["gn"][0] == free[1]["gn"][0]
    assert snaps[1]["gn"][0] >= 4 * max_norm
    flags = []
    for k in range(5):
        lr = _table(case)[min(k, 3)]
        flags.append(_check_step(snaps[k], snaps[k + 1], k + 1, lr, case, max_norm, tag=f"{kind} {case} step {k}"))
        assert snaps[k + 1]["gn"][1] == sum(flags), (k, snaps[k + 1]["gn"], flags)  # the counter, step by step
        assert snaps[k + 1]["step"] == k + 1 and np.isfinite(snaps[k + 1]["loss"])
    assert flags[0] and sum(flags) >= 1
    print(f"{kind} {case}: max_norm {max_norm!r}, clipped {flags}")
    assert not torch.equal(snaps[1]["params"], free[1]["params"])  # the clipping changed the first update
    if CASES[case][2] is not None:  # EMA on top: the average follows the clipped parameters
        from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
        from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at, ema_reference
        for k in range(5):
            d = ema_decay_at(k, CASES[case][2], True)
            for name, (off, shape) in LAYOUT.items():
                sl = slice(off, off + int(np.prod(shape)))
                err = _rel(snaps[k + 1]["ema"][sl].double().numpy(),
                           ema_reference(snaps[k]["ema"][sl], snaps[k + 1]["params"][sl], d))
                assert err <= TOL, (kind, k, name, err)


# ---- graph replay -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sgd", "adamw"])
@pytest.mark.parametrize("kind", list(ENGINES))
def test_graph_replay_equals_eager_steps(gpu, kind, case):
    """One 4-step graph replay (k_grad_sqnorm and the CLIP form inside the captured graph) is bitwise the four eager
    steps, counter and norm included.  Then a new limit between two replays of the same captured graph: the second
    replay, at 1e30, clips nothing and is bitwise four eager steps taken after the same switch."""
    max_norm = _limit(kind, case)
    snaps = _eager_steps(kind, case, max_norm)
    dtype, persistent = ENGINES[kind]

    def run(graph):
        _, eng = _engine(dtype, persistent, _opt(case, max_norm))
        if graph:
            eng.run(B, 4, graph=True)
        else:
            for _ in range(4):
                eng.run(B, 1, graph=False)
        first = _snap(eng)
        eng.set_max_grad_norm(OFF)
        assert eng.cfg.optimizer.max_grad_norm == OFF
        if graph:
            eng.run(B, 4, graph=True)
        else:
            for _ in range(4):
                eng.run(B, 1, graph=False)
        second = _snap(eng)
        eng.check_errors()
        eng.close()
        return first, second
    g1, g2 = run(True)
    e1, e2 = run(False)
    for got in (g1, e1):
        assert got["step"] == 4 and got["gn"] == snaps[4]["gn"] and got["gn"][1] >= 1
        for key in ("params", "m", "v", "grads"):
            assert got[key] is None if snaps[4][key] is None else torch.equal(got[key], snaps[4][key]), key
        assert got["loss"] == snaps[4]["loss"]
    assert g2["step"] == 8 and g2["gn"] == e2["gn"]
    assert g2["gn"][1] == g1["gn"][1], "the second replay ran at 1e30: no further step may count as clipped"
    for key in ("params", "m", "v", "grads"):
        assert g2[key] is None if e2[key] is None else torch.equal(g2[key], e2[key]), key


def test_switching_and_readout_errors(gpu):
    """set_max_grad_norm(None) switches the form off (the run is then the unclipped one), bad limits are refused and
    leave the engine as it was, grad_norm() needs clipping on, reset clears the counter only."""
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    max_norm = _limit("sliced-bf16", "sgd")
    free = _eager_steps("sliced-bf16", "sgd", None)
    _, eng = _engine("bf16", True, _opt("sgd", max_norm))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            eng.set_max_grad_norm(bad)
    assert eng.cfg.optimizer.max_grad_norm == max_norm
    eng.set_max_grad_norm(None)
    assert eng.clip_part is None and eng.cfg.optimizer.max_grad_norm is None
    with pytest.raises(RuntimeError, match="clipping"):
        eng.grad_norm()
    eng.run(B, 2, graph=True)
    got = _snap(eng)
    assert torch.equal(got["params"], free[2]["params"]) and torch.equal(got["m"], free[2]["m"])
    eng.set_max_grad_norm(max_norm)
    eng.run(B, 1, graph=True)
    norm, n = eng.grad_norm(reset=True)
    assert norm > max_norm and n == 1 and eng.grad_norm() == (norm, 0)
    eng.close()
    with pytest.raises(ValueError):
        _engine("bf16", True, OptimizerConfig(momentum=0.9, max_grad_norm=0.0))


# ---- two ranks sharing one GPU --------------------------------------------------------------------------------
def _rank_worker(rank, ws, port, dtype, persistent, comm, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["DCA_XGMI_TIMEOUT_S"] = "30"  # a protocol bug ends as an error flag, not a hang
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.data.sampler import distributed_indices
        from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.ddp import FusedDDPTrainer, broadcast_module_state
        from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        data, labels = synthetic_cifar(NDATA, seed=5)
        order = distributed_indices(NDATA, ws, rank)
        torch.manual_seed(100 + rank)
        model = NetResDeep()
        broadcast_module_state(model, 0)
        model = model.to(dev)
        tr = None
        if comm == "xgmi":
            tr = FusedDDPTrainer(model, data.to(dev), labels.to(dev), batch_max=B, dtype=dtype, persistent=persistent,
                                 comm="xgmi", max_indices=len(order), optimizer=_opt("adamw", OFF))
            assert tr.comm == "xgmi", tr.comm
            eng = tr.engine
        else:
            eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                                   EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, world_size=ws,
                                                rank=rank, comm="external", optimizer=_opt("adamw", OFF)))
        eng.set_indices(order)
        eng.set_cursor(0)
        eng.read_loss(reset=True)

        def allreduce(t):
            h = t.cpu()
            dist.all_reduce(h)
            t.copy_(h.to(t.device))

        prev = _snap(eng)
        max_norm, flags = OFF, []
        for k in range(3):
            if comm == "xgmi":
                eng.run(B, 1)  # graph-captured: step, reduction, all-reduce (sum only), norm kernel, optimiser pass
            else:
                eng.run_external(B, 1, allreduce)
            cur = _snap(eng)
            # engine.grads holds the gradient summed over the ranks; the norm is that of the average
            flags.append(_check_step(prev, cur, k + 1, TABLE[k], "adamw", max_norm, inv_ws=1.0 / ws,
                                     tag=f"rank {rank} {comm} step {k}"))
            assert cur["step"] == k + 1 and cur["gn"][1] == sum(flags)
            for key in ("params", "m", "v", "grads"):
                other = cur[key].clone()
                dist.broadcast(other, 0)
                assert torch.equal(cur[key], other), (key, k)
            both = torch.tensor([cur["gn"][0], float(cur["gn"][1])], dtype=torch.float64)
            dist.broadcast(both, 0)
            assert both.tolist() == [cur["gn"][0], float(cur["gn"][1])]
            if k == 0:  # from here on a limit that clips, the same on both ranks; the captured graph stays
                max_norm = 0.25 * cur["gn"][0]
                eng.set_max_grad_norm(max_norm)
            prev = cur
        assert flags[0] is False and flags[1] is True, flags
        eng.check_errors()
        assert eng.read_loss()[1] == 3
        if tr is not None:
            tr.close()
        else:
            dist.barrier()
            eng.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("comm", ["xgmi", "external"])
@pytest.mark.parametrize("dtype,persistent", [("bf16", True), ("fp32", False)], ids=["sliced", "multikernel"])
def test_two_ranks_one_gpu(gpu, port, dtype, persistent, comm):
    spawn_ranks(_rank_worker, 2, lambda r: (r, 2, port, dtype, persistent, comm))


# ---- k_sqnorm_part / k_clip_coef and the gscale forms of k_sgd / k_adam ---------------------------------------------
SIZES = [1, 255, 257, 524288 + 257]


def _state_words(state):
    host = state[:2].cpu()
    return float(host[0]), host.view(torch.float32)[2].numpy().copy(), int(host.view(torch.int32)[3])


@pytest.mark.parametrize("n", SIZES)
def test_clip_coef_kernels(gpu, n):
    """Slices that start 4 bytes past a 16-byte boundary (scalar head, float4 body, scalar tail; the largest runs the
    grid-stride loop): N within 1e-10 of float64, coef the oracle's float bit for bit, below and above the limit; the
    counter counts the clipping calls; one NaN gives a NaN coef; the gradient itself keeps its bits."""
    from distributeddataparallel_cifar10_amd.ops.functional import clip_coef_, clip_readout, clip_scale, clip_state
    from distributeddataparallel_cifar10_amd.utils.schedule import clip_reference
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(n)
    host = torch.randn(n + 9, generator=gen)
    buf = host.to(dev)
    assert buf.data_ptr() % 16 == 0
    g = buf[1:1 + n]
    true = float(np.sqrt(np.sum(host[1:1 + n].double().numpy() ** 2)))
    state = clip_state(dev)
    expect = 0
    for max_norm in (4.0 * true, 0.25 * true, 0.999999 * true):
        norm, coef = clip_reference(host[1:1 + n], max_norm)
        gs = clip_coef_(g, max_norm, state)
        assert gs.data_ptr() == state.data_ptr() + 8 and gs.dtype == torch.float32 and gs.numel() == 1
        got_norm, got_coef, count = _state_words(state)
        expect += int(coef < 1)
        print(f"n = {n}, max_norm {max_norm!r}: norm {got_norm!r} (float64 {norm!r}), coef {float(got_coef)!r}")
        assert abs(got_norm - norm) <= TOL_NORM * norm, (got_norm, norm)
        assert got_coef.tobytes() == coef.tobytes(), (float(got_coef), float(coef))
        assert count == expect and float(clip_scale(state).cpu()) == float(coef)
    assert expect == 2 and clip_readout(state, reset=True) == (got_norm, 2) and clip_readout(state) == (got_norm, 0)
    assert torch.equal(buf.cpu(), host)
    buf[1 + n // 2] = float("nan")
    clip_coef_(g, 1.0, state)
    got_norm, got_coef, count = _state_words(state)
    assert np.isnan(got_norm) and np.isnan(got_coef) and count == 0
    with pytest.raises(ValueError):
        clip_coef_(g, 0.0, state)
    with pytest.raises(TypeError):
        clip_coef_(g, 1.0, state[:2])


@pytest.mark.parametrize("n", SIZES)
def test_update_kernels_with_gscale(gpu, n):
    """sgd_step_ and adam_step_ with the coefficient of clip_coef_ as `gscale`, on slices 4 bytes past a 16-byte
    boundary, against the oracles on the clipped gradient ((a) and (b) above); with gscale=None the results are bitwise
    those of a call without the argument."""
    from distributeddataparallel_cifar10_amd.ops.functional import (adam_state, adam_step_, clip_coef_, clip_state,
                                                                  sgd_step_)
    from distributeddataparallel_cifar10_amd.utils.schedule import adam_reference, clip_reference, sgd_reference
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3 * n + 1)
    sl = slice(1, 1 + n)
    # parameters of rms 0.25, a gradient of rms 1 clipped to a quarter of its norm
    host = {"p": 0.25 * torch.randn(n + 9, generator=gen), "g": torch.randn(n + 9, generator=gen),
            "m": 0.1 * torch.randn(n + 9, generator=gen), "v": 0.1 * torch.rand(n + 9, generator=gen)}
    max_norm = 0.25 * float(host["g"][sl].double().norm())
    norm, coef = clip_reference(host["g"][sl], max_norm)
    assert coef < 1
    x = _clipped(host["g"][sl], coef)
    lr, wd = 0.1, 5e-4

    def dev_bufs():
        return {k: t.to(dev) for k, t in host.items()}
    p0 = host["p"][sl].double().numpy()

    def check(got, want, keys, what):
        for key, a, b in zip(keys, got, want):
            assert _rel(a, b) <= TOL, (what, key, _rel(a, b))
        d_want = want[0] - p0
        assert _rel(got[0] - p0, d_want) <= TOL_DELTA, (what, _rel(got[0] - p0, d_want))
        print(f"n = {n} {what}: (a) {max(_rel(a, b) for a, b in zip(got, want)):.3e}, "
              f"(b) {_rel(got[0] - p0, d_want):.3e}")

    # SGD with momentum and weight decay (the buffer initialised: first = 0)
    bufs, state = dev_bufs(), clip_state(dev)
    first = torch.zeros(1, dtype=torch.int32, device=dev)
    gs = clip_coef_(bufs["g"][sl], max_norm, state)
    sgd_step_(bufs["p"][sl], bufs["g"][sl], lr, MU, wd, buf=bufs["m"][sl], first=first, gscale=gs)
    want = sgd_reference(p0, x, host["m"][sl], lr, MU, wd)
    check([bufs[k][sl].double().cpu().numpy() for k in ("p", "m")], want, ("p", "m"), "sgd")
    for k in ("p", "m", "g"):  # outside the slice, and the gradient: bit for bit what they were
        out = bufs[k].cpu()
        assert torch.equal(out[:1], host[k][:1]) and torch.equal(out[1 + n:], host[k][1 + n:]), k
    assert torch.equal(bufs["g"].cpu(), host["g"])
    # AdamW and Adam (L2), step 1
    for decoupled, awd in ((True, 5e-2), (False, 5e-4)):
        bufs, st = dev_bufs(), adam_state(dev)
        adam_step_(bufs["p"][sl], bufs["g"][sl], bufs["m"][sl], bufs["v"][sl], st, lr, BETAS, EPS, awd,
                   decoupled=decoupled, gscale=gs)
        want = adam_reference(p0, x, host["m"][sl], host["v"][sl], 1, lr, BETAS[0], BETAS[1], EPS, awd, decoupled)
        check([bufs[k][sl].double().cpu().numpy() for k in ("p", "m", "v")], want, ("p", "m", "v"),
              "adamw" if decoupled else "adam")
        for k in ("p", "m", "v"):
            out = bufs[k].cpu()
            assert torch.equal(out[:1], host[k][:1]) and torch.equal(out[1 + n:], host[k][1 + n:]), k
    # gscale=None: the calls as they were
    a, b = dev_bufs(), dev_bufs()
    sgd_step_(a["p"][sl], a["g"][sl], lr, MU, wd, buf=a["m"][sl], first=None)
    sgd_step_(b["p"][sl], b["g"][sl], lr, MU, wd, buf=b["m"][sl], first=None, gscale=None)
    sa, sb = adam_state(dev), adam_state(dev)
    adam_step_(a["p"][sl], a["g"][sl], a["m"][sl], a["v"][sl], sa, lr, BETAS, EPS, 5e-2)
    adam_step_(b["p"][sl], b["g"][sl], b["m"][sl], b["v"][sl], sb, lr, BETAS, EPS, 5e-2, gscale=None)
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(sa, sb)
    with pytest.raises(TypeError):
        sgd_step_(a["p"][sl], a["g"][sl], lr, gscale=torch.ones(2, device=dev))
    with pytest.raises(TypeError):
        adam_step_(a["p"][sl], a["g"][sl], a["m"][sl], a["v"][sl], sa, lr, gscale=torch.ones(1, device=dev).double())


# ---- entry points ----------------------------------------------------------------------------------------------------
def _records(path):
    return [x for x in map(json.loads, open(path).read().splitlines()) if "epoch" in x]


def _check_records(recs, limit, steps):
    assert [x["steps"] for x in recs] == steps and all(np.isfinite(x["loss"]) and x["loss"] > 0 for x in recs)
    for x in recs:
        assert x["clip_grad_norm"] == limit and x["grad_norm"] > 0 and np.isfinite(x["grad_norm"])
        assert isinstance(x["clipped_steps"], int) and 0 <= x["clipped_steps"] <= x["steps"]
        assert x["clipped_steps"] >= int(limit / (x["grad_norm"] + 1e-6) < 1.0)  # the last step's norm is in the record


def test_main_entry_points_with_clipping(gpu, tmp_path):
    """main.py --clip-grad-norm on the fused engine (AdamW) and on the ops engine (FlatAdam, k_sqnorm_part + k_clip_coef
    + k_adam's gscale form): the metrics records, and no file beyond those of the same run without the flag."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for name, extra in (("fused", []), ("ops", ["--engine", "ops"])):
        out = tmp_path / name
        out.mkdir()
        mj = out / "m.json"
        r = subprocess.run([sys.executable, "main.py", "--world-size", "1", "--synthetic", "512", "--epochs", "2",
                            "--max-steps", "8", "--optimizer", "adamw", "--weight-decay", "0.05", "--clip-grad-norm",
                            "0.05", "--port", str(free_port()), "--checkpoint-path",
                            str(out / "birds_vs_airplanes.pt"), "--metrics-json", str(mj), *extra],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert re.search(r"Epoch 1, Training loss \d", r.stdout), r.stdout
        recs = _records(str(mj))
        _check_records(recs, 0.05, [8, 8])
        assert recs[0]["engine"] in (("ops",) if extra else ("sliced", "multikernel"))
        assert sorted(os.listdir(out)) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                           "birds_vs_airplanes.pt.optim.pt", "m.json"]
        side = torch.load(str(out / "birds_vs_airplanes.pt.optim.pt"), weights_only=True)
        assert sorted(side) == (["exp_avg", "exp_avg_sq", "kind", "step"] if extra else
                                ["engine", "exp_avg", "exp_avg_sq", "kind", "step"])


def _main_flow(tmp, name, **kw):
    """main.py's per-rank flow at world size 1 with --synthetic 512 --max-steps 8 --optimizer adamw --weight-decay 0.05
    --lr 2e-3 --lr-schedule cosine --clip-grad-norm 0.05; returns the final checkpoint's path and the optimiser state
    (the sidecar's content)."""
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint
    dev = torch.device("cuda", 0)
    cfg = TrainConfig(synthetic=512, epochs=2, max_steps=8, optimizer="adamw", weight_decay=0.05, lr=2e-3,
                      lr_schedule="cosine", clip_grad_norm=0.05, **kw)
    data, labels = load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=dev,
                          sampler="distributed", seed=0, set_epoch=cfg.set_epoch)
    torch.manual_seed(21)
    model = build_model_for_rank(cfg, 0, 1, dev, data, labels, loader)
    try:
        try:
            train_loop(model, loader, 0, cfg)
        except RuntimeError as ex:
            if "injected failure" not in str(ex):
                raise
        assert model.engine.cfg.optimizer.max_grad_norm == 0.05
        st = model.engine.optimizer_state()
        assert st["step"] == 16 or kw.get("fail_at_step")
        side = {key: {k: v.detach().cpu().clone() for k, v in st[key].items()} for key in ("exp_avg", "exp_avg_sq")}
        side["step"], side["norm"] = st["step"], model.engine.grad_norm()[0]
        final = save_checkpoint(model, os.path.join(tmp, name + "_final.pt"), 0)
    finally:
        model.close()
    return final, side


def test_resume_gives_the_same_checkpoint_and_sidecar(gpu, tmp_path):
    """Two epochs straight against one epoch + --resume on the fused engine with clipping: bitwise equal final
    checkpoint, moments and last norm -- clipping carries no state of its own; the sidecar holds nothing new."""
    tmp = str(tmp_path)
    mj = os.path.join(tmp, "a.json")
    a, side_a = _main_flow(tmp, "a", checkpoint_path=os.path.join(tmp, "a.pt"), metrics_json=mj)
    _check_records(_records(mj), 0.05, [8, 8])
    leg = os.path.join(tmp, "b.pt")
    _main_flow(tmp, "b1", checkpoint_path=leg, fail_at_step=9)  # epoch 1 (8 steps, checkpoint), stopped at step 9
    assert json.load(open(leg + ".meta.json")) == {"epoch": 1, "step": 8, "opt_step": 8}
    assert sorted(torch.load(leg + ".optim.pt", weights_only=True)) == ["engine", "exp_avg", "exp_avg_sq", "kind",
                                                                        "step"]
    b, side_b = _main_flow(tmp, "b2", resume=leg, checkpoint=False)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert side_a["step"] == side_b["step"] == 16 and side_a["norm"] == side_b["norm"] > 0
    for key in ("exp_avg", "exp_avg_sq"):
        for k in side_a[key]:
            assert torch.equal(side_a[key][k], side_b[key][k]), (key, k)
            assert float(side_a[key][k].abs().sum()) > 0
