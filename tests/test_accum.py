"""Gradient accumulation without a GPU: the oracle ``utils/schedule.accumulate_reference`` against torch's usual loop
(``(loss / K).backward()`` K times), ``GradAccumulator`` on a plain module and over ``FlatBucketDDP`` (gloo, 2 ranks)
against torch DDP running that loop with SGD-momentum and with AdamW + ``clip_grad_norm_``, the flag's validation and
the schedule's conversion to optimiser steps, and ``main_no_ddp.py --accumulate-steps 2`` on the CPU with its metrics
records, the dropped micro-steps and ``--resume`` in mid-window."""
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

from distributeddataparallel_cifar10_amd.utils.schedule import accumulate_reference

CPU = torch.device("cpu")


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _linear_window(K, seed=0, batch=5):
    """A small nn.Linear and K batches: the K per-micro-step gradients (each from a zeroed .grad) and the gradient
    torch's loop leaves, ``(loss / K).backward()`` K times into one .grad."""
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(13, 7)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    batches = [(torch.randn(batch, 13, generator=g), torch.randint(0, 7, (batch,), generator=g)) for _ in range(K)]
    singles = []
    for x, y in batches:
        lin.zero_grad()
        F.cross_entropy(lin(x), y).backward()
        singles.append([p.grad.detach().clone() for p in lin.parameters()])
    lin.zero_grad()
    for x, y in batches:
        (F.cross_entropy(lin(x), y) / K).backward()
    return singles, [p.grad.detach().clone() for p in lin.parameters()]


@pytest.mark.parametrize("K", [2, 4])
def test_accumulate_reference_is_torchs_loop_bitwise(K):
    """K a power of two: dividing the loss by K scales every micro-step's gradient exactly, so torch's accumulated
    .grad and the rule (sum in order, one multiplication by fp32(1 / K)) hold the same bits."""
    singles, loop = _linear_window(K, seed=K)
    for i, want in enumerate(loop):
        g32, g64 = accumulate_reference([s[i] for s in singles], K)
        assert g32.dtype == np.float32 and g64.dtype == np.float64 and g32.shape == tuple(want.shape)
        assert g32.tobytes() == want.numpy().tobytes()
        assert np.abs(g32 - g64).max() <= K * 2.0 ** -24 * np.abs(g64).max() + 1e-45
        assert np.abs(g32).max() > 0


def test_accumulate_reference_k3_within_the_rounding_bound():
    """K = 3: 1 / 3 is not a power of two, so the two sides round differently; each makes at most 2K roundings of
    magnitudes bounded by sum_k |g_k| / K: elementwise |diff| <= 4K * 2^-24 * sum_k |g_k| / K.  One sample per
    micro-step, so that a weight gradient is one product and the bias gradient one term: with several samples the two
    sides' batch sums (a dot product over the batch of terms scaled before, or after, it) round terms larger than
    |g_k| where they cancel, which is the matrix product's error and not the accumulation's."""
    K = 3
    singles, loop = _linear_window(K, seed=5, batch=1)
    worst = 0.0
    for i, want in enumerate(loop):
        g32, g64 = accumulate_reference([s[i] for s in singles], K)
        bound = 4 * K * 2.0 ** -24 * sum(np.abs(s[i].double().numpy()) for s in singles) / K
        diff = np.abs(g32.astype(np.float64) - want.double().numpy())
        worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all(), float((diff - bound).max())
        assert (np.abs(g64 - want.double().numpy()) <= bound).all()
    print(f"K = 3: worst |diff| / bound {worst:.3f}")


def test_accumulate_reference_arguments():
    g = [np.ones(4, dtype=np.float32), np.full(4, 2.0, dtype=np.float32)]
    g32, g64 = accumulate_reference(g, 2)
    assert g32.tolist() == [1.5] * 4 and g64.tolist() == [1.5] * 4
    one32, _ = accumulate_reference(g[:1], 1)
    assert one32.tobytes() == g[0].tobytes()
    with pytest.raises(ValueError):
        accumulate_reference(g, 3)  # a window of 3 needs 3 gradients
    for bad in (0, -1, 1.5, None, float("nan"), True):
        with pytest.raises(ValueError):
            accumulate_reference(g, bad)
    # inf / NaN propagate as in IEEE arithmetic
    bad32, _ = accumulate_reference([np.array([np.inf, 1.0], np.float32), np.array([-np.inf, np.nan], np.float32)], 2)
    assert np.isnan(bad32).all()


# ---- GradAccumulator -------------------------------------------------------------------------------------------------
MAX_NORM = 0.1
K_WIN, WINDOWS = 2, 2


def _pair(kind, a_params, b_params, flat=None):
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatSGD
    if kind == "sgd":
        opt_a = FlatSGD(flat, lr=1e-2, momentum=0.9, weight_decay=5e-4) if flat is not None else \
            torch.optim.SGD(a_params, lr=1e-2, momentum=0.9, weight_decay=5e-4)
        return opt_a, torch.optim.SGD(b_params, lr=1e-2, momentum=0.9, weight_decay=5e-4), None
    kw = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2)
    opt_a = FlatAdam(flat, max_grad_norm=MAX_NORM, **kw) if flat is not None else torch.optim.AdamW(a_params, **kw)
    return opt_a, torch.optim.AdamW(b_params, **kw), MAX_NORM


def _run_both(kind, ours, a, theirs, b, rank, flat):
    """K_WIN x WINDOWS micro-steps: `ours` through GradAccumulator (zeroed gradient, backward, accumulate; clip and step
    on the window's last micro-step), `theirs` through torch's loop.  The accumulation buffer is poisoned with NaN
    between the windows: a window's first micro-step overwrites it."""
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import GradAccumulator
    opt_a, opt_b, max_norm = _pair(kind, a.parameters(), b.parameters(), ours if flat else None)
    acc = GradAccumulator(ours, K_WIN)
    assert acc.micro == 0 and acc.steps == K_WIN
    snap = [p.detach().clone() for p in a.parameters()]
    stepped = []
    for step in range(K_WIN * WINDOWS):
        g = torch.Generator().manual_seed(1000 * step + rank)
        x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
        loss = F.cross_entropy(ours(x), y)
        opt_a.zero_grad()
        loss.backward()
        last = acc.accumulate()
        stepped.append(last)
        if last:
            if max_norm is not None and not flat:  # (FlatAdam clips inside step())
                torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm)
            opt_a.step()
            for buf in acc.state().values():
                buf.fill_(float("nan"))
        else:  # a micro-step inside the window changes no parameter
            for p, q in zip(a.parameters(), snap):
                assert torch.equal(p, q)
        (F.cross_entropy(theirs(x), y) / K_WIN).backward()
        if last:
            if max_norm is not None:
                norm = float(torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm))
                if flat:
                    assert abs(opt_a.last_grad_norm() - norm) <= 1e-4 * norm, (step, opt_a.last_grad_norm(), norm)
            opt_b.step()
            opt_b.zero_grad()
            snap = [p.detach().clone() for p in a.parameters()]
    assert stepped == [False, True] * WINDOWS and acc.micro == 0
    # the bounds of tests/test_clip.py's comparison with torch DDP
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.isfinite(pa).all(), n
        assert torch.allclose(pa, pb, atol=1e-5, rtol=1e-4), (n, float((pa - pb).abs().max()))
        if kind == "adamw" and flat:
            off = (pa.data_ptr() - ours.flat.data_ptr()) // 4
            m = opt_a.exp_avg[off:off + pa.numel()].view(pa.shape)
            assert torch.allclose(m, opt_b.state[pb]["exp_avg"], atol=1e-6, rtol=1e-4), n


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_grad_accumulator_plain_module_matches_torch_loop(kind):
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    torch.manual_seed(3)
    base = NetResDeep()
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    _run_both(kind, a, a, b, b, 0, flat=False)


def _flat_worker(rank, ws, port, kind, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatBucketDDP
        torch.manual_seed(3)
        base = NetResDeep()
        a, b = copy.deepcopy(base), copy.deepcopy(base)
        ours = FlatBucketDDP(a, bucket_cap_mb=0.1)
        theirs = torch.nn.parallel.DistributedDataParallel(b)
        _run_both(kind, ours, a, theirs, b, rank, flat=True)
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
def test_grad_accumulator_gloo_matches_torch_ddp(port, kind):
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


def test_grad_accumulator_rule_and_overlap():
    """On the CPU the buffer holds the oracle's bits after every micro-step (K = 3), the last one leaves the mean in the
    gradient too, a NaN-filled buffer is overwritten; overlap=True optimisers are refused."""
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD, GradAccumulator
    ddp = FlatBucketDDP(NetResDeep())
    acc = GradAccumulator(ddp, 3)
    buf = acc._acc[None]
    buf.fill_(float("nan"))
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(ddp.flat_grad.shape, generator=gen) for _ in range(3)]
    for k, g in enumerate(grads):
        ddp.flat_grad.copy_(g)
        last = acc.accumulate()
        assert last == (k == 2) and not torch.isnan(buf).any()
        if not last:
            want = grads[0].numpy() if k == 0 else (grads[0].numpy() + grads[1].numpy()).astype(np.float32)
            assert buf.numpy().tobytes() == want.tobytes() and torch.equal(ddp.flat_grad, g)
    g32, _ = accumulate_reference(grads, 3)
    assert buf.numpy().tobytes() == g32.tobytes() and ddp.flat_grad.numpy().tobytes() == g32.tobytes()
    assert acc.micro == 0 and set(acc.state()) == {n for n, _ in ddp.module.named_parameters()}
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            GradAccumulator(ddp, bad)
    for cls in (FlatSGD, FlatAdam):
        d2 = FlatBucketDDP(NetResDeep())
        cls(d2, overlap=True)
        with pytest.raises(ValueError, match="overlap"):
            GradAccumulator(d2, 2)
    late = GradAccumulator(ddp, 2)
    FlatSGD(ddp, overlap=True)
    with pytest.raises(ValueError, match="overlap"):
        late.accumulate()


def test_later_entry_points_are_claimed_by_a_gpu_test():
    """tests/test_ops_nn_refs.py's coverage table lists what ops/_native.py's `_declare` holds; an entry point added
    since is declared in LATER_ENTRY_POINTS, and held here to the same rule: a GPU test module names the wrapper that
    calls it, the wrapper calls it, and the library's source exports it."""
    from distributeddataparallel_cifar10_amd.ops import _native as N
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.dirname(os.path.abspath(N.__file__))
    claimed = {"dca_ops_grad_accum": ("test_accum_gpu.py", "grad_accum_(")}
    assert set(N.LATER_ENTRY_POINTS) == set(claimed)
    wrappers = open(os.path.join(pkg, "functional.py")).read()
    exported = open(os.path.join(pkg, "..", "csrc", "ops_api.hip")).read()
    for name, (module, token) in claimed.items():
        text = open(os.path.join(here, module)).read()
        assert "pytest.mark.gpu" in text and token in text, (name, module, token)
        assert f"N.lib().{name}(" in wrappers and f"int {name}(" in exported, name


# ---- flags -----------------------------------------------------------------------------------------------------------
def _parse(argv):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser()).parse_args(argv), "data/CIFAR-10/")


def test_flag_and_config_validation(monkeypatch, capsys):
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.runtime import engine as E
    cfg = _parse([])
    assert cfg.accumulate_steps == 1 and not T.optimizer_active(cfg) and T.engine_optimizer(cfg, 10) is None
    for bad in ("0", "-3", "1.5", "two"):
        with pytest.raises(SystemExit):
            _parse(["--accumulate-steps", bad])
    capsys.readouterr()
    for bad in (0, -1, 1.5, True, None, float("nan")):
        with pytest.raises(ValueError):
            E.check_optimizer_config(E.OptimizerConfig(accumulate_steps=bad))
    E.check_optimizer_config(E.OptimizerConfig(accumulate_steps=4))
    # the flag alone turns the split form on, and the engine's config carries K
    cfg = _parse(["--accumulate-steps", "4"])
    assert T.optimizer_active(cfg)
    on = T.engine_optimizer(cfg, 8)
    assert (on.kind, on.momentum, on.accumulate_steps, on.max_grad_norm) == ("sgd", 0.0, 4, None)
    # K = 1 is off: the same TrainConfig, and with another option on the constructor receives what it did without it
    assert _parse(["--accumulate-steps", "1"]) == _parse([])
    made = []
    real = E.OptimizerConfig

    def spy(**kw):
        made.append(kw)
        return real(**kw)
    monkeypatch.setattr(E, "OptimizerConfig", spy)
    T.engine_optimizer(_parse(["--momentum", "0.9"]), 5)
    T.engine_optimizer(_parse(["--momentum", "0.9", "--accumulate-steps", "1"]), 5)
    T.engine_optimizer(_parse(["--momentum", "0.9", "--accumulate-steps", "2"]), 5)
    assert "accumulate_steps" not in made[0] and made[2]["accumulate_steps"] == 2
    assert list(made[0]) == list(made[1]) and all(np.array_equal(made[0][k], made[1][k]) for k in made[0])


def test_k1_builds_what_no_flag_builds(monkeypatch):
    """A generic backend with --accumulate-steps 1 constructs no GradAccumulator and the optimisers of the run without
    the flag."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel import flat_ddp
    made = []

    class SpySGD(torch.optim.SGD):
        def __init__(self, params, **kw):
            made.append(("torch", kw))
            super().__init__(params, **kw)

    class SpyFlat(flat_ddp.FlatSGD):
        def __init__(self, ddp, *a, **kw):
            made.append(("flat", a, kw))
            super().__init__(ddp, *a, **kw)

    class SpyAcc(flat_ddp.GradAccumulator):
        def __init__(self, model, steps):
            made.append(("accum", steps))
            super().__init__(model, steps)

    monkeypatch.setattr(torch.optim, "SGD", SpySGD)
    monkeypatch.setattr(flat_ddp, "FlatSGD", SpyFlat)
    monkeypatch.setattr(flat_ddp, "GradAccumulator", SpyAcc)
    data, labels = synthetic_cifar(32, seed=0)
    loader = DeviceLoader(data, labels, batch_size=16, world_size=1, rank=0, device="cpu")
    for k in (1, 2):
        made.clear()
        run = T.TrainConfig(epochs=1, checkpoint=False, lr=0.02, accumulate_steps=k)
        T.train_loop(NetResDeep(), loader, 0, run)
        T.train_loop(flat_ddp.FlatBucketDDP(NetResDeep()), loader, 0, run)
        if k == 1:
            assert made == [("torch", {"lr": 0.02}), ("flat", (0.02,), {})], made
        else:
            assert [m[0] for m in made] == ["torch", "accum", "flat", "accum"] and made[1] == ("accum", 2), made


@pytest.mark.parametrize("epochs,spe,K", [(3, 7, 2), (2, 5, 3)])
def test_table_counts_optimiser_steps(epochs, spe, K):
    """(epochs * steps_per_epoch) // K entries; --lr-step-epochs E decays every E * steps_per_epoch // K optimiser
    steps; --lr-warmup-steps counts optimiser steps."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.utils.schedule import lr_table
    base = ["--epochs", str(epochs), "--accumulate-steps", str(K)]
    assert len(T.lr_table_for(_parse(base), spe)) == epochs * spe // K
    assert len(T.lr_table_for(_parse(base + ["--max-steps", "4"]), spe)) == epochs * 4 // K
    assert len(T.lr_table_for(_parse(["--epochs", "1", "--accumulate-steps", "50"]), spe)) == 1  # at least one entry
    got = T.lr_table_for(_parse(base + ["--lr-schedule", "step", "--lr-step-epochs", "1", "--lr-warmup-steps", "2"]), spe)
    want = lr_table("step", 1e-2, epochs * spe // K, warmup_steps=2, step_size=spe // K, gamma=0.1)
    assert np.array_equal(got, want)
    assert got[0] == 1e-2 / 3 and got[2] == 1e-2
    if 2 + spe // K < len(got):
        assert got[2 + spe // K] == pytest.approx(1e-3)
    assert len(T.engine_optimizer(_parse(base), spe).lr_table) == epochs * spe // K


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
        if "accum_micro" in meta:
            cfg.extra["accum_micro"] = meta["accum_micro"]
        for _ in range(meta["epoch"]):  # this loader's shuffle is one seeded stream: skip the orders already used
            loader.indices()
    M.training_loop(model, loader)
    return model


# 256 images at batch 64, 3 of the 4 steps per epoch, 3 epochs: 9 micro-steps, windows of 2 straddle the epochs
ACC = ["--synthetic", "256", "--momentum", "0.9", "--accumulate-steps", "2", "--max-steps", "3", "--epochs", "3",
       "--lr-schedule", "cosine"]


def _records(path):
    return [r for r in map(json.loads, open(path).read().splitlines()) if "epoch" in r]


def test_main_no_ddp_accumulate_metrics_and_resume(tmp_path, monkeypatch, capsys):
    """The metrics fields; optimiser steps per epoch 1, 2, 1 and one dropped micro-step on stderr; the checkpoint after
    epoch 1 is in mid-window (accum_micro 1, "accum" in the sidecar) and --resume from it ends bitwise where the
    uninterrupted run ends; another K is refused with both values named."""
    from distributeddataparallel_cifar10_amd.utils.schedule import lr_table
    mj, mj_off = str(tmp_path / "on.json"), str(tmp_path / "off.json")
    b = str(tmp_path / "b" / "birds_vs_airplanes.pt")
    capsys.readouterr()
    straight = _no_ddp_run(monkeypatch, 5, ACC + ["--no-checkpoint", "--metrics-json", mj])
    err = capsys.readouterr().err
    assert "--accumulate-steps 2" in err and "last 1 micro-step" in err, err
    recs = _records(mj)
    table = lr_table("cosine", 1e-2, 4)  # 9 // 2 optimiser steps
    assert [r["steps"] for r in recs] == [3, 3, 3] and [r["optimizer_steps"] for r in recs] == [1, 2, 1]
    assert [r["accumulate_steps"] for r in recs] == [2, 2, 2]
    assert [r["lr"] for r in recs] == [table[0], table[2], table[3]]  # the last optimiser step taken
    off = _no_ddp_run(monkeypatch, 5, ["--synthetic", "256", "--momentum", "0.9", "--max-steps", "3", "--epochs", "1",
                                       "--no-checkpoint", "--metrics-json", mj_off])
    assert "accumulate" not in capsys.readouterr().err
    for r in _records(mj_off):
        assert r["accumulate_steps"] is None and r["optimizer_steps"] == r["steps"] == 3
    assert any(not torch.equal(v, off.state_dict()[k]) for k, v in straight.state_dict().items())

    with pytest.raises(RuntimeError, match="injected failure"):
        _no_ddp_run(monkeypatch, 5, ACC + ["--checkpoint-path", b, "--fail-at-step", "4"])
    assert json.load(open(b + ".meta.json")) == {"epoch": 1, "step": 3, "opt_step": 1, "accum_micro": 1}
    side = torch.load(b + ".optim.pt", weights_only=True)
    assert sorted(side) == ["accum", "accumulate_steps", "momentum_buffer", "step"]
    assert side["step"] == 1 and side["accumulate_steps"] == 2 and len(side["accum"]) == 9
    assert all(float(v.abs().sum()) > 0 for v in side["accum"].values())
    resumed = _no_ddp_run(monkeypatch, 99, ACC + ["--resume", b, "--no-checkpoint"])
    assert "last 1 micro-step" in capsys.readouterr().err
    sa, sb = straight.state_dict(), resumed.state_dict()
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    other = [a if a != "2" else "3" for a in ACC]
    with pytest.raises(SystemExit) as ex:
        _no_ddp_run(monkeypatch, 99, other + ["--resume", b, "--no-checkpoint"])
    assert "--accumulate-steps 2" in str(ex.value) and "--accumulate-steps 3" in str(ex.value)
