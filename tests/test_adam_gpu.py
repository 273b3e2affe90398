"""Adam / AdamW on an MI355X: the Adam forms of the fused engine's optimiser pass (csrc/optimizer.hip k_apply_adam)
against the float64 oracle ``utils/schedule.adam_reference`` -- every update, the update's own increment, the state, the
derived weight copies, graph replay, restored bias state, EMA on top, two ranks on one GPU, the untouched SGD forms --,
the flat ops kernel ``k_adam`` through ``adam_step_`` / ``FlatAdam``, and the entry point with resume.

Engine cases: 256 synthetic images, batch 8 (the pass's size is the fixed 76,140-float buffer).  Bounds, per tensor:

* (a) p', m', v' <= 1e-6 relative L2: each takes about six fp32 roundings of <= 6e-8 against float64 and the fp32
  beta2 another 6e-8 -- <= 5e-7 summed linearly;
* (b) the increment p' - p <= 1e-4 relative L2 against the oracle's: the fp32 rounding of p' relative to the
  increment, 6e-8 * |p| / |increment| (<= 1.5e-5 while rms(increment) >= 0.3 * lr; the test asserts >= 0.1 * lr, so
  the bound is not vacuous), plus the arithmetic of (a)."""
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
BETAS = (0.9, 0.999)
NDATA, B = 256, 8
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}
CASES = {"adamw": ("adamw", 5e-2, 1e-8), "adamw-eps1e-3": ("adamw", 5e-2, 1e-3), "adam-l2": ("adam", 5e-4, 1e-8)}
TOL, TOL_DELTA = 1e-6, 1e-4
OFF_RS, FLAT_N = 76076, 76140


def _opt(case="adamw", **kw):
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    kind, wd, eps = CASES[case]
    return OptimizerConfig(kind=kind, weight_decay=wd, eps=eps, betas=BETAS, lr_table=TABLE, **kw)


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
                rs=torch.cat([eng.bn.running_mean, eng.bn.running_var]).detach().cpu().clone(),
                step=eng.optimizer_step(), loss=eng.read_loss()[0])


@functools.lru_cache(maxsize=None)
def _eager_steps(kind, case, ema=None):
    """Five single eager steps; the state before and after every step."""
    dtype, persistent = ENGINES[kind]
    extra = {} if ema is None else dict(ema_decay=ema, ema_warmup=True)
    _, eng = _engine(dtype, persistent, _opt(case, **extra))
    assert eng.kind_name == ("sliced" if persistent else "multikernel")
    snaps = [_snap(eng)]
    for _ in range(5):
        eng.run(B, 1, graph=False)
        snaps.append(_snap(eng))
    eng.check_errors()
    eng.close()
    return snaps


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def _check_update(prev, cur, t, lr, case, inv_ws=1.0, tag=""):
    """cur = adam_reference(prev state, cur's grads, t): (a) p', m', v' and (b) the increment p' - p, per tensor."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.schedule import adam_reference
    kind, wd, eps = CASES[case]
    worst, worst_d, least = 0.0, 0.0, np.inf
    for name, (off, shape) in LAYOUT.items():
        sl = slice(off, off + int(np.prod(shape)))
        p0 = prev["params"][sl].double().numpy()
        want = adam_reference(p0, cur["grads"][sl], prev["m"][sl], prev["v"][sl], t, lr, BETAS[0], BETAS[1], eps, wd,
                              kind == "adamw", inv_ws)
        got = [cur[k][sl].double().numpy() for k in ("params", "m", "v")]
        errs = [_rel(g, w) for g, w in zip(got, want)]
        d_want = want[0] - p0
        rms = float(np.sqrt(np.mean(d_want ** 2)))
        d_err = _rel(got[0] - p0, d_want)
        worst, worst_d, least = max(worst, *errs), max(worst_d, d_err), min(least, rms / lr)
        assert rms >= 0.1 * lr, (tag, name, "the oracle's increment is too small for bound (b)", rms, lr)
        for what, err in zip(("param", "exp_avg", "exp_avg_sq"), errs):
            assert err <= TOL, (tag, name, what, err)
        assert d_err <= TOL_DELTA, (tag, name, "increment", d_err)
        assert float(cur["grads"][sl].abs().sum()) > 0, (tag, name, "no gradient")
    print(f"{tag}: worst relative L2 (a) {worst:.3e}, (b) {worst_d:.3e}; least rms(increment) / lr {least:.3f}")


def _pads_zero(snap):
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    used = torch.zeros(OFF_RS, dtype=torch.bool)
    for off, shape in LAYOUT.values():
        used[off:off + int(np.prod(shape))] = True
    assert int((~used).sum()) > 0
    for key in ("params", "m", "v"):
        pad = snap[key][:OFF_RS][~used]
        assert torch.equal(pad, torch.zeros_like(pad)) and not bool(torch.signbit(pad).any()), key


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(ENGINES))
def test_per_step_update_matches_reference(gpu, kind, case):
    snaps = _eager_steps(kind, case)
    s0 = snaps[0]
    assert s0["step"] == 0 and float(s0["m"].abs().sum()) == 0.0 and float(s0["v"].abs().sum()) == 0.0
    for k in range(5):
        lr = TABLE[min(k, len(TABLE) - 1)]  # the fifth step holds the last table entry
        _check_update(snaps[k], snaps[k + 1], k + 1, lr, case, tag=f"{kind} {case} step {k}")
        cur = snaps[k + 1]
        assert cur["step"] == k + 1 and np.isfinite(cur["loss"])
        for key in ("params", "m", "v"):
            assert bool(torch.isfinite(cur[key]).all()), key
        assert float(cur["v"].min()) >= 0.0
        _pads_zero(cur)


@pytest.mark.parametrize("kind", list(ENGINES))
def test_derived_copies_follow_the_update(gpu, kind):
    """A twin that re-derives every kernel-layout weight copy from the fp32 parameters after each step: bitwise the
    same after four steps."""
    snaps = _eager_steps(kind, "adamw")
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt())
    for _ in range(4):
        eng.run(B, 1, graph=False)
        eng.derive()
    twin = _snap(eng)
    eng.close()
    for key in ("params", "m", "v"):
        assert torch.equal(twin[key], snaps[4][key]), key
    assert twin["loss"] == snaps[4]["loss"], (twin["loss"], snaps[4]["loss"])


@pytest.mark.parametrize("kind", list(ENGINES))
def test_graph_replay_equals_eager_steps(gpu, kind):
    """One 4-step graph replay (table, step counter, running products and hyper-parameters read from device memory) is
    bitwise the four eager steps."""
    snaps = _eager_steps(kind, "adamw")
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt())
    eng.run(B, 4, graph=True)
    got = _snap(eng)
    eng.close()
    assert got["step"] == 4
    for key in ("params", "m", "v"):
        assert torch.equal(got[key], snaps[4][key]), key
    assert got["loss"] == snaps[4]["loss"], (got["loss"], snaps[4]["loss"])


def test_graph_replay_picks_up_a_new_table(gpu):
    """Adam with weight decay 0: a second replay of the captured graph after set_lr_table([0] * 8) leaves the
    parameters where they are while the moments move."""
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    _, eng = _engine("bf16", True, OptimizerConfig(kind="adam", betas=BETAS, lr_table=TABLE))
    eng.run(B, 4, graph=True)
    got = _snap(eng)
    eng.set_lr_table([0.0] * 8)
    eng.run(B, 4, graph=True)
    after = _snap(eng)
    eng.close()
    assert got["step"] == 4 and after["step"] == 8
    assert torch.equal(after["params"], got["params"])
    assert not torch.equal(after["m"], got["m"]) and not torch.equal(after["v"], got["v"])


@pytest.mark.parametrize("kind", ["sliced-bf16", "multikernel-fp32"])
def test_restored_state_continues_with_the_bias_of_its_step(gpu, kind):
    """load_optimizer_state with step 3 (moments of the eager run): the next update is the oracle's at t = 4 -- the
    running products were restored with the counter.  A state of another kind is refused with both kinds named."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT, OptimizerConfig
    snaps = _eager_steps(kind, "adamw")
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt())

    def views(flat):
        return {n: flat[o:o + int(np.prod(s))].view(s) for n, (o, s) in LAYOUT.items()}
    state = {"step": 3, "kind": "adamw", "exp_avg": views(snaps[3]["m"]), "exp_avg_sq": views(snaps[3]["v"])}
    with pytest.raises(ValueError, match=r"'sgd'.*'adamw'"):
        eng.load_optimizer_state({"step": 3, "momentum_buffer": views(snaps[3]["m"])})
    with pytest.raises(ValueError):
        eng.load_optimizer_state({"step": 3, "kind": "adamw", "exp_avg": {}, "exp_avg_sq": {}})
    eng.load_optimizer_state(state)
    got = eng.optimizer_state()
    assert got["step"] == 3 and got["kind"] == "adamw" and sorted(got) == ["exp_avg", "exp_avg_sq", "kind", "step"]
    for n in LAYOUT:
        assert torch.equal(got["exp_avg"][n].cpu(), state["exp_avg"][n])
        assert torch.equal(got["exp_avg_sq"][n].cpu(), state["exp_avg_sq"][n])
    prev = _snap(eng)
    eng.run(B, 1, graph=False)
    cur = _snap(eng)
    eng.close()
    assert cur["step"] == 4
    _check_update(prev, cur, 4, TABLE[3], "adamw", tag=f"{kind} restored step 3")
    sgd_eng = _engine(dtype, persistent, OptimizerConfig(momentum=0.9, lr_table=TABLE))[1]
    with pytest.raises(ValueError, match=r"'adamw'.*'sgd'"):
        sgd_eng.load_optimizer_state(state)
    sgd_eng.close()


@pytest.mark.parametrize("kind", list(ENGINES))
def test_ema_with_adamw(gpu, kind):
    """The EMA form on top of AdamW: every EMA update against utils/ema's float64 oracle, and the training is bitwise
    the AdamW run without EMA."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at, ema_reference
    with_ema, without = _eager_steps(kind, "adamw", 0.3), _eager_steps(kind, "adamw")
    assert torch.equal(with_ema[0]["ema"][:OFF_RS], with_ema[0]["params"][:OFF_RS])
    for k in range(6):
        for key in ("params", "m", "v", "rs"):
            assert torch.equal(with_ema[k][key], without[k][key]), (k, key)
        assert with_ema[k]["loss"] == without[k]["loss"] and with_ema[k]["step"] == without[k]["step"] == k
    for k in range(5):
        prev, cur, d = with_ema[k], with_ema[k + 1], ema_decay_at(k, 0.3, True)
        worst = 0.0
        for name, (off, shape) in LAYOUT.items():
            sl = slice(off, off + int(np.prod(shape)))
            err = _rel(cur["ema"][sl].double().numpy(), ema_reference(prev["ema"][sl], cur["params"][sl], d))
            worst = max(worst, err)
            assert err <= TOL, (kind, k, name, err)
        rs = slice(OFF_RS, OFF_RS + 64)
        err = _rel(cur["ema"][rs].double().numpy(), ema_reference(prev["ema"][rs], cur["rs"], d))
        print(f"{kind} step {k}: d = {d:.6f}, worst relative L2 {max(worst, err):.3e}")
        assert err <= TOL, (kind, k, "running statistics", err)


@pytest.mark.parametrize("kind", ["sliced-bf16", "multikernel-fp32"])
def test_sgd_is_untouched(gpu, kind):
    """OptimizerConfig(kind="sgd", momentum=0.9, ...) for five steps: bitwise the run built without the new field, and
    bitwise the same after Adam was switched on and off again with set_optimizer before the first step."""
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    dtype, persistent = ENGINES[kind]
    sgd = dict(momentum=0.9, weight_decay=5e-4, lr_table=[0.01, 0.02, 0.03, 0.015])

    def five(eng):
        eng.run(B, 5, graph=True)
        s = _snap(eng)
        eng.close()
        return s
    plain = five(_engine(dtype, persistent, OptimizerConfig(**sgd))[1])
    named = five(_engine(dtype, persistent, OptimizerConfig(kind="sgd", **sgd))[1])
    _, eng = _engine(dtype, persistent, OptimizerConfig(kind="sgd", **sgd))
    eng.set_optimizer(_opt("adamw"))
    assert eng.exp_avg_sq is not None and eng.optimizer_state()["kind"] == "adamw"
    eng.set_optimizer(OptimizerConfig(kind="sgd", **sgd))
    assert sorted(eng.optimizer_state()) == ["momentum_buffer", "step"]
    switched = five(eng)
    for other in (named, switched):
        assert other["step"] == plain["step"] == 5 and other["loss"] == plain["loss"]
        for key in ("params", "m", "grads"):
            assert torch.equal(other[key], plain[key]), key
    none = _engine(dtype, persistent, OptimizerConfig(**sgd))[1]
    assert none.exp_avg_sq is None  # nothing allocated for SGD
    with pytest.raises(ValueError, match="momentum"):
        none.set_optimizer(OptimizerConfig(kind="adam", momentum=0.9))
    assert none.exp_avg_sq is None and none.cfg.optimizer.kind == "sgd"
    none.close()


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
                                 comm="xgmi", max_indices=len(order), optimizer=_opt())
            assert tr.comm == "xgmi", tr.comm
            eng = tr.engine
        else:
            eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                                   EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, world_size=ws,
                                                rank=rank, comm="external", optimizer=_opt()))
        eng.set_indices(order)
        eng.set_cursor(0)
        eng.read_loss(reset=True)

        def allreduce(t):
            h = t.cpu()
            dist.all_reduce(h)
            t.copy_(h.to(t.device))

        prev = _snap(eng)
        for k in range(3):
            if comm == "xgmi":
                eng.run(B, 1)  # graph-captured: step, reduction, all-reduce (sum only), optimiser pass
            else:
                eng.run_external(B, 1, allreduce)
            cur = _snap(eng)
            # engine.grads holds the gradient summed over the ranks; the update averages it
            _check_update(prev, cur, k + 1, TABLE[k], "adamw", inv_ws=1.0 / ws, tag=f"rank {rank} {comm} step {k}")
            assert cur["step"] == k + 1
            for key in ("params", "m", "v", "grads"):
                other = cur[key].clone()
                dist.broadcast(other, 0)
                assert torch.equal(cur[key], other), (key, k)
            prev = cur
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


# ---- k_adam through adam_step_ / FlatAdam ------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("n", [1, 255, 257, 524288 + 257])
def test_adam_step_kernel(gpu, n, decoupled):
    """Three steps of adam_step_ on slices that start at element offsets 0..3 of larger buffers (scalar head, float4
    body, scalar tail; the largest length runs the grid-stride loop) against adam_reference with the bounds above; the
    elements outside the slice keep their bits."""
    from distributeddataparallel_cifar10_amd.ops.functional import adam_state, adam_step_
    from distributeddataparallel_cifar10_amd.utils.schedule import adam_reference
    dev = torch.device("cuda", 0)
    wd, eps, lrs = (5e-2 if decoupled else 5e-4), 1e-8, [2e-3, 4e-3, 6e-3]
    g = torch.Generator().manual_seed(n)
    worst, worst_d = 0.0, 0.0
    for off in range(4):
        total = n + off + 5
        # parameters of rms 0.25 (a trained layer's scale: bound (b) carries 6e-8 * |p| / |increment|)
        host = {"p": 0.25 * torch.randn(total, generator=g), "g": torch.randn(total, generator=g)}
        host["m"], host["v"] = torch.full((total,), 0.25), torch.full((total,), 0.5)  # sentinels outside the slice
        host["m"][off:off + n] = 0
        host["v"][off:off + n] = 0
        bufs = {k: t.to(dev) for k, t in host.items()}
        state = adam_state(dev)
        ref = [host[k][off:off + n].double().numpy() for k in ("p", "m", "v")]
        for t, lr in enumerate(lrs, start=1):
            grad = torch.randn(n, generator=g)
            bufs["g"][off:off + n].copy_(grad)
            before = bufs["p"][off:off + n].double().cpu().numpy()
            adam_step_(bufs["p"][off:off + n], bufs["g"][off:off + n], bufs["m"][off:off + n], bufs["v"][off:off + n],
                       state, lr, BETAS, eps, wd, decoupled=decoupled)
            want = adam_reference(before, grad, ref[1], ref[2], t, lr, BETAS[0], BETAS[1], eps, wd, decoupled)
            got = [bufs[k][off:off + n].double().cpu().numpy() for k in ("p", "m", "v")]
            for what, a, b in zip(("p", "m", "v"), got, want):
                err = _rel(a, b)
                worst = max(worst, err)
                assert err <= TOL, (off, t, what, err)
            d_want = want[0] - before
            assert float(np.sqrt(np.mean(d_want ** 2))) >= 0.1 * lr
            d_err = _rel(got[0] - before, d_want)
            worst_d = max(worst_d, d_err)
            assert d_err <= TOL_DELTA, (off, t, d_err)
            ref = [got[0], got[1], got[2]]
        assert state.cpu().tolist() == [3.0, BETAS[0] * BETAS[0] * BETAS[0], BETAS[1] * BETAS[1] * BETAS[1]]
        for k in ("p", "m", "v"):  # outside the slice: bit for bit what it was
            out = bufs[k].cpu()
            assert torch.equal(out[:off], host[k][:off]) and torch.equal(out[off + n:], host[k][off + n:]), (k, off)
    print(f"n = {n}: worst relative L2 (a) {worst:.3e}, (b) {worst_d:.3e}")


def test_adam_step_rejects_bad_arguments(gpu):
    from distributeddataparallel_cifar10_amd.ops.functional import adam_state, adam_step_
    dev = torch.device("cuda", 0)
    p, g, m, v = (torch.zeros(8, device=dev) for _ in range(4))
    st = adam_state(dev)
    with pytest.raises(ValueError):
        adam_step_(p, g, m, v, st, 1e-3, (0.9, 1.0))
    with pytest.raises(ValueError):
        adam_step_(p, g, m, v, st, 1e-3, eps=0.0)
    with pytest.raises(TypeError):
        adam_step_(p, g, m, v[:4], st, 1e-3)
    with pytest.raises(TypeError):
        adam_step_(p, g, m, v, st.float(), 1e-3)
    assert st.cpu().tolist() == [0.0, 1.0, 1.0]


def test_flat_adam_overlap_matches_step(gpu):
    """FlatAdam on a small FlatBucketDDP model: the per-bucket updates of overlap=True (slices of the flat buffer, the
    step state advanced once by step()) give the parameters of the one-kernel step() -- the same arithmetic per
    element, so bitwise -- and both follow torch.optim.AdamW."""
    import torch.nn as nn
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    def net():
        return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Flatten(), nn.Linear(8 * 8 * 8, 10)).to(dev)
    a, b, c = net(), net(), net()
    b.load_state_dict(a.state_dict())
    c.load_state_dict(a.state_dict())
    da = FlatBucketDDP(a, bucket_cap_mb=0.005, first_bucket_mb=0.002)
    db = FlatBucketDDP(b, bucket_cap_mb=0.005, first_bucket_mb=0.002)
    assert len(da.buckets) >= 2
    kw = dict(lr=2e-3, betas=BETAS, eps=1e-8, weight_decay=5e-2)
    oa, ob = FlatAdam(da, **kw), FlatAdam(db, overlap=True, **kw)
    oc = torch.optim.AdamW(c.parameters(), **kw)
    for step in range(4):
        g = torch.Generator().manual_seed(10 * step)
        x, y = torch.randn(4, 3, 8, 8, generator=g).to(dev), torch.randint(0, 10, (4,), generator=g).to(dev)
        for d, o in ((da, oa), (db, ob), (c, oc)):
            o.zero_grad()
            nn.functional.cross_entropy(d(x), y).backward()
            o.step()
        torch.cuda.synchronize()
        assert torch.equal(db.flat, da.flat), step
        assert torch.equal(ob.exp_avg, oa.exp_avg) and torch.equal(ob.exp_avg_sq, oa.exp_avg_sq), step
    assert oa.steps_taken() == ob.steps_taken() == 4
    for pa, pc in zip(a.parameters(), c.parameters()):
        torch.testing.assert_close(pa, pc, rtol=1e-4, atol=1e-6)


# ---- entry point ---------------------------------------------------------------------------------------------------
def test_main_entry_point_with_adamw(gpu, tmp_path):
    mj = tmp_path / "m.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "main.py", "--world-size", "1", "--synthetic", "512", "--epochs", "2",
                        "--max-steps", "8", "--optimizer", "adamw", "--weight-decay", "0.05", "--lr-schedule",
                        "cosine", "--eval", "--port", str(free_port()), "--checkpoint-path",
                        str(tmp_path / "birds_vs_airplanes.pt"), "--metrics-json", str(mj)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Epoch 1, Training loss \d", r.stdout) and "Test accuracy" in r.stdout, r.stdout
    from distributeddataparallel_cifar10_amd.utils.schedule import lr_table
    table = lr_table("cosine", 1e-2, 16)
    recs = [x for x in map(json.loads, mj.read_text().splitlines()) if "epoch" in x]
    assert [x["steps"] for x in recs] == [8, 8] and all(np.isfinite(x["loss"]) and x["loss"] > 0 for x in recs)
    assert [x["lr"] for x in recs] == [table[7], table[15]]
    assert sorted(os.listdir(tmp_path)) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                            "birds_vs_airplanes.pt.optim.pt", "m.json"]
    assert len(torch.load(str(tmp_path / "birds_vs_airplanes.pt"), weights_only=True)) == 66
    side = torch.load(str(tmp_path / "birds_vs_airplanes.pt.optim.pt"), weights_only=True)
    assert sorted(side) == ["engine", "exp_avg", "exp_avg_sq", "kind", "step"]
    assert side["kind"] == "adamw" and side["step"] == 8 and len(side["exp_avg"]) == len(side["exp_avg_sq"]) == 9


def _main_flow(tmp, name, **kw):
    """main.py's per-rank flow at world size 1 with --synthetic 512 --max-steps 8 --optimizer adamw --weight-decay 0.05
    --lr 2e-3 --lr-schedule cosine; writes the final state as a checkpoint and returns its path and the final
    moments."""
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint
    dev = torch.device("cuda", 0)
    cfg = TrainConfig(synthetic=512, epochs=2, max_steps=8, optimizer="adamw", weight_decay=0.05, lr=2e-3,
                      lr_schedule="cosine", **kw)
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
        st = model.engine.optimizer_state()
        assert st["step"] == 16 or kw.get("fail_at_step")
        moments = {key: {k: v.detach().cpu().clone() for k, v in st[key].items()} for key in ("exp_avg", "exp_avg_sq")}
        final = save_checkpoint(model, os.path.join(tmp, name + "_final.pt"), 0)
    finally:
        model.close()
    return final, moments


def _ops_flow(monkeypatch, seed, **kw):
    """main.py's per-rank flow at world size 1 on the ops engine (FlatBucketDDP + FlatAdam, k_adam) with --synthetic 256
    --max-steps 4 --optimizer adamw; returns the final state_dict and the optimiser."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.utils.checkpoint import export_state_dict
    dev = torch.device("cuda", 0)
    cfg = T.TrainConfig(synthetic=256, max_steps=4, engine="ops", optimizer="adamw", weight_decay=0.05, lr=2e-3,
                        lr_schedule="cosine", **kw)
    data, labels = T.load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=dev,
                          sampler="distributed", seed=0)
    made, real = [], T.make_adam
    monkeypatch.setattr(T, "make_adam", lambda m, c: made.append(real(m, c)) or made[-1])
    torch.manual_seed(seed)
    model = T.build_model_for_rank(cfg, 0, 1, dev, data, labels, loader)
    try:
        T.train_loop(model, loader, 0, cfg)
    except RuntimeError as ex:
        if "injected failure" not in str(ex):
            raise
    finally:
        monkeypatch.setattr(T, "make_adam", real)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in export_state_dict(model).items()}, made[0]


def test_ops_engine_resume_adamw(gpu, tmp_path, monkeypatch):
    """The ops engine (FlatAdam on k_adam): two epochs straight against one epoch + --resume -- bitwise equal final
    state and moments, the device step state restored with the counter."""
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam
    leg = str(tmp_path / "b.pt")
    straight, opt_a = _ops_flow(monkeypatch, 5, epochs=2, checkpoint=False)
    _ops_flow(monkeypatch, 5, epochs=2, checkpoint_path=leg, fail_at_step=5)  # epoch 1 of the same schedule
    side = torch.load(leg + ".optim.pt", weights_only=True)
    assert sorted(side) == ["exp_avg", "exp_avg_sq", "kind", "step"] and side["step"] == 4 and side["kind"] == "adamw"
    resumed, opt_b = _ops_flow(monkeypatch, 99, epochs=2, resume=leg, checkpoint=False)
    assert isinstance(opt_a, FlatAdam) and isinstance(opt_b, FlatAdam)
    assert opt_a.steps_taken() == opt_b.steps_taken() == 8
    assert torch.equal(opt_a._state.cpu(), opt_b._state.cpu())
    assert list(straight) == list(resumed)
    for k in straight:
        assert torch.equal(straight[k], resumed[k]), k
    assert torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq)
    assert float(opt_a.exp_avg_sq.abs().sum()) > 0


def test_resume_gives_the_same_checkpoint_and_moments(gpu, tmp_path):
    """Two epochs straight against one epoch + --resume on the fused engine (AdamW, cosine over both epochs): bitwise
    equal final checkpoint, exp_avg and exp_avg_sq; a sidecar of the other kind ends the run by name."""
    tmp = str(tmp_path)
    a, mom_a = _main_flow(tmp, "a", checkpoint_path=os.path.join(tmp, "a.pt"))
    leg = os.path.join(tmp, "b.pt")
    _main_flow(tmp, "b1", checkpoint_path=leg, fail_at_step=9)  # epoch 1 (8 steps, checkpoint), stopped at step 9
    assert json.load(open(leg + ".meta.json")) == {"epoch": 1, "step": 8, "opt_step": 8}
    b, mom_b = _main_flow(tmp, "b2", resume=leg, checkpoint=False)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for key in ("exp_avg", "exp_avg_sq"):
        for k in mom_a[key]:
            assert torch.equal(mom_a[key][k], mom_b[key][k]), (key, k)
            assert float(mom_a[key][k].abs().sum()) > 0
    side = torch.load(leg + ".optim.pt", weights_only=True)
    torch.save({"step": 8, "momentum_buffer": side["exp_avg"], "engine": side["engine"]}, leg + ".optim.pt")
    with pytest.raises(SystemExit, match=r"--optimizer sgd.*--optimizer adamw"):
        _main_flow(tmp, "b3", resume=leg, checkpoint=False)
