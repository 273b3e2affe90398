"""Global gradient-norm clipping without a GPU: the float64 oracle ``utils/schedule.clip_reference`` against
``torch.nn.utils.clip_grad_norm_``, ``FlatSGD`` / ``FlatAdam(max_grad_norm=...)`` on the CPU (gloo, 2 ranks) against
torch's ``SGD`` / ``AdamW`` + ``clip_grad_norm_`` under torch DDP, the flag's validation, and ``main_no_ddp.py
--clip-grad-norm`` on the CPU with its metrics records and ``--resume``."""
import argparse
import copy
import json
import os
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from distributeddataparallel_cifar10_amd.utils.schedule import clip_reference

CPU = torch.device("cpu")


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _torch_clip(grads, max_norm):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(total), [p.grad for p in ps]


@pytest.mark.parametrize("case", ["below", "above"])
def test_clip_reference_matches_torch(case):
    """fp64 inputs: the norm to rtol 1e-12; the coefficient is torch's, rounded once to fp32 (exactly 1.0 below the
    limit); torch's clipped gradient is g * coef to the fp32 rounding of coef (2^-24 < 6e-8 relative)."""
    g = torch.Generator().manual_seed(7)
    grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((32, 2048), (10, 32), (32,), (32, 3, 3, 3))]
    true = float(torch.sqrt(sum((x * x).sum() for x in grads)))
    max_norm = 2.0 * true if case == "below" else 0.25 * true
    norm, coef = clip_reference(grads, max_norm)
    want, clipped = _torch_clip(grads, max_norm)
    assert abs(norm - want) <= 1e-12 * want and abs(norm - true) <= 1e-12 * true
    assert isinstance(coef, np.float32)
    if case == "below":
        assert coef == np.float32(1.0) and coef.tobytes() == np.float32(1.0).tobytes()
        for x, c in zip(grads, clipped):
            assert torch.equal(x, c)
    else:
        assert coef == np.float32(max_norm / (want + 1e-6)) and coef < 1
        for x, c in zip(grads, clipped):
            torch.testing.assert_close(c, x * float(coef), rtol=6e-8, atol=0.0)
    # one tensor instead of a list, and the averaging of a summed gradient
    flat = torch.cat([x.reshape(-1) for x in grads])
    assert clip_reference(flat, max_norm)[0] == pytest.approx(norm, rel=1e-14)
    half, c2 = clip_reference([2.0 * x for x in grads], max_norm, inv_ws=0.5)
    assert half == pytest.approx(norm, rel=1e-14) and c2 == coef


def test_clip_reference_nan_and_bad_limits():
    g = torch.randn(100, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    g[17] = float("nan")
    norm, coef = clip_reference([g, torch.ones(3, dtype=torch.float64)], 1.0)
    want, clipped = _torch_clip([g], 1.0)
    assert np.isnan(norm) and np.isnan(want) and np.isnan(coef) and isinstance(coef, np.float32)
    assert bool(torch.isnan(clipped[0]).all())  # torch's clamp(max=1) keeps the NaN: so does the oracle
    for bad in (0.0, -1.0, float("nan"), None):
        with pytest.raises(ValueError):
            clip_reference([g], bad)
    # fp32 inputs: the averaged gradient is rounded to fp32 first, as the kernels form it
    x = torch.tensor([1.0 + 2.0 ** -23, 3.0], dtype=torch.float32)
    n32, _ = clip_reference(x, 1.0, inv_ws=1.0 / 3.0)
    y = (x.double().numpy() * (1.0 / 3.0)).astype(np.float32).astype(np.float64)
    assert n32 == float(np.sqrt(np.sum(y * y)))


# ---- FlatSGD / FlatAdam on the CPU ----------------------------------------------------------------------------------
MAX_NORM = 0.1


def _flat_worker(rank, ws, port, kind, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD
        torch.manual_seed(3)
        base = NetResDeep()
        a, b = copy.deepcopy(base), copy.deepcopy(base)
        ours = FlatBucketDDP(a, bucket_cap_mb=0.1)
        theirs = torch.nn.parallel.DistributedDataParallel(b)
        if kind == "sgd":
            opt_a = FlatSGD(ours, lr=1e-2, momentum=0.9, weight_decay=5e-4, max_grad_norm=MAX_NORM)
            opt_b = torch.optim.SGD(b.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
        else:
            opt_a = FlatAdam(ours, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2, max_grad_norm=MAX_NORM)
            opt_b = torch.optim.AdamW(b.parameters(), lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2)
        assert opt_a.last_grad_norm() == 0.0 and opt_a.clipped_steps() == 0
        clipped = 0
        for step in range(3):
            g = torch.Generator().manual_seed(1000 * step + rank)
            x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
            loss = F.cross_entropy(ours(x), y)
            opt_a.zero_grad()
            loss.backward()
            opt_a.step()
            loss = F.cross_entropy(theirs(x), y)
            opt_b.zero_grad()
            loss.backward()
            norm = float(torch.nn.utils.clip_grad_norm_(b.parameters(), MAX_NORM))
            opt_b.step()
            clipped += int(MAX_NORM / (norm + 1e-6) < 1.0)
            assert abs(opt_a.last_grad_norm() - norm) <= 1e-4 * norm, (step, opt_a.last_grad_norm(), norm)
        assert clipped >= 1 and opt_a.clipped_steps() == clipped, (clipped, opt_a.clipped_steps())
        assert opt_a.clipped_steps(reset=True) == clipped and opt_a.clipped_steps() == 0
        # the bounds of test_flat_ddp's SGD comparison and test_adam's (the two all-reduces sum in different orders)
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert torch.allclose(pa, pb, atol=1e-5, rtol=1e-4), (n, float((pa - pb).abs().max()))
            if kind == "adamw":
                off = (pa.data_ptr() - ours.flat.data_ptr()) // 4
                m = opt_a.exp_avg[off:off + pa.numel()].view(pa.shape)
                assert torch.allclose(m, opt_b.state[pb]["exp_avg"], atol=1e-6, rtol=1e-4), n
        other = ours.flat.clone()
        dist.broadcast(other, 0)
        assert torch.equal(other, ours.flat)  # the ranks stay in step
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_flat_optimizers_gloo_match_torch_with_clipping(port, kind):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_flat_worker, args=(r, 2, port, kind, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in res if r[1]]
    assert not bad, "\n".join(f"rank {r}:\n{e}" for r, e in bad)


def test_overlap_with_max_grad_norm_raises():
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD
    ddp = FlatBucketDDP(NetResDeep())
    for cls in (FlatSGD, FlatAdam):
        with pytest.raises(ValueError, match="overlap"):
            cls(ddp, overlap=True, max_grad_norm=1.0)
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError):
                cls(ddp, max_grad_norm=bad)
    assert ddp._fused_opt is None  # nothing was registered by the refused constructions
    assert FlatSGD(ddp).max_grad_norm is None and FlatAdam(ddp).max_grad_norm is None


# ---- flags -----------------------------------------------------------------------------------------------------------
def _parse(argv):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser()).parse_args(argv), "data/CIFAR-10/")


def test_flag_and_config_validation():
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig, check_optimizer_config
    cfg = _parse([])
    assert cfg.clip_grad_norm is None and not T.optimizer_active(cfg) and T.engine_optimizer(cfg, 10) is None
    cfg = _parse(["--clip-grad-norm", "0.5"])
    assert cfg.clip_grad_norm == 0.5 and T.optimizer_active(cfg)  # the flag alone: the split step form
    on = T.engine_optimizer(cfg, 5)
    assert (on.kind, on.momentum, on.weight_decay, on.ema_decay, on.max_grad_norm) == ("sgd", 0.0, 0.0, None, 0.5)
    assert set(on.lr_table) == {1e-2}
    assert T.engine_optimizer(_parse(["--momentum", "0.9"]), 5).max_grad_norm is None
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            _parse(["--clip-grad-norm", bad])
    check_optimizer_config(OptimizerConfig(max_grad_norm=2.0))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            check_optimizer_config(OptimizerConfig(max_grad_norm=bad))
    # the generic engines' optimisers receive the value
    flat = FlatBucketDDP(NetResDeep())
    sgd = T.make_optimizer(flat, cfg, [1e-2])
    adam = T.make_optimizer(flat, _parse(["--clip-grad-norm", "0.5", "--optimizer", "adamw"]), [1e-2])
    assert isinstance(sgd, FlatSGD) and sgd.max_grad_norm == 0.5
    assert isinstance(adam, FlatAdam) and adam.max_grad_norm == 0.5
    assert T.make_optimizer(flat, _parse(["--momentum", "0.9"]), [1e-2]).max_grad_norm is None


# ---- main_no_ddp.py on the CPU -----------------------------------------------------------------------------------
def _no_ddp_run(monkeypatch, seed, argv):
    """main_no_ddp.py's flow on the CPU with `argv`; returns the trained module."""
    import main_no_ddp as M
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    from distributeddataparallel_cifar10_amd.utils.checkpoint import load_checkpoint
    cfg = config_from_args(add_cli_args(argparse.ArgumentParser(), batch_default=64).parse_args(argv), M.data_path)
    monkeypatch.setattr(M, "_cfg", cfg)
    monkeypatch.setattr(M, "device", CPU)
    torch.manual_seed(seed)
    model = NetResDeep()
    loader = M.prepare()
    if cfg.resume:
        meta = load_checkpoint(model, cfg.resume, strict=True, map_location=CPU)  # (as train.build_model_for_rank)
        cfg.extra.update(start_epoch=meta["epoch"] + 1, start_step=meta["step"], opt_step=meta["opt_step"])
        for _ in range(meta["epoch"]):  # this loader's shuffle is one seeded stream: skip the orders already used
            loader.indices()
    M.training_loop(model, loader)
    return model


CLIP = ["--synthetic", "256", "--momentum", "0.9", "--clip-grad-norm", "0.05"]


def _records(path):
    return [r for r in map(json.loads, open(path).read().splitlines()) if "epoch" in r]


def test_main_no_ddp_clip_metrics_and_resume(tmp_path, monkeypatch):
    """main_no_ddp.py --synthetic 256 --momentum 0.9 --clip-grad-norm 0.05 on the CPU: the three metrics fields; with
    the flag off they are null like the other optional fields; the clipped run differs from the unclipped one; two
    epochs straight equal one epoch + --resume bitwise, with no file beyond those of a momentum run."""
    mj, mj_off = str(tmp_path / "on.json"), str(tmp_path / "off.json")
    b = str(tmp_path / "b" / "birds_vs_airplanes.pt")
    straight = _no_ddp_run(monkeypatch, 5, CLIP + ["--epochs", "2", "--no-checkpoint", "--metrics-json", mj])
    recs = _records(mj)
    assert [r["steps"] for r in recs] == [4, 4]
    for r in recs:
        assert r["clip_grad_norm"] == 0.05 and r["grad_norm"] > 0 and np.isfinite(r["grad_norm"])
        assert isinstance(r["clipped_steps"], int) and 0 <= r["clipped_steps"] <= r["steps"]
        # the last step's norm decides whether that step counted
        assert r["clipped_steps"] >= int(0.05 / (r["grad_norm"] + 1e-6) < 1.0)
    off = _no_ddp_run(monkeypatch, 5, ["--synthetic", "256", "--momentum", "0.9", "--epochs", "2", "--no-checkpoint",
                                       "--metrics-json", mj_off])
    for r in _records(mj_off):
        assert r["grad_norm"] is None and r["clipped_steps"] is None and r["clip_grad_norm"] is None
        assert r["ema_decay"] is None  # (how the other optional fields are written)
    if sum(r["clipped_steps"] for r in recs):
        assert any(not torch.equal(v, off.state_dict()[k]) for k, v in straight.state_dict().items())

    with pytest.raises(RuntimeError, match="injected failure"):
        _no_ddp_run(monkeypatch, 5, CLIP + ["--epochs", "2", "--checkpoint-path", b, "--fail-at-step", "5"])
    assert sorted(os.listdir(tmp_path / "b")) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                                  "birds_vs_airplanes.pt.optim.pt"]
    side = torch.load(b + ".optim.pt", weights_only=True)
    assert sorted(side) == ["momentum_buffer", "step"] and side["step"] == 4  # nothing new in the sidecar
    resumed = _no_ddp_run(monkeypatch, 99, CLIP + ["--epochs", "2", "--resume", b, "--no-checkpoint"])
    sa, sb = straight.state_dict(), resumed.state_dict()
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
