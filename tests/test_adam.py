"""Adam / AdamW without a GPU: the float64 oracle ``utils/schedule.adam_reference`` against torch's own optimisers,
``FlatAdam`` on the CPU (gloo, 2 ranks) against ``torch.optim.AdamW`` on a plain replica, the flags' validation, and
``main_no_ddp.py --optimizer adamw`` on the CPU with its ``.optim.pt`` sidecar and ``--resume``."""
import argparse
import copy
import os
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from distributeddataparallel_cifar10_amd.utils.schedule import adam_reference

CPU = torch.device("cpu")


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("wd", [0.0, 5e-2])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_adam_reference_matches_torch(decoupled, wd, eps):
    """10 steps on random float64 tensors: <= 1e-12 relative against torch.optim.Adam / AdamW."""
    g = torch.Generator().manual_seed(7)
    p = torch.randn(3, 41, dtype=torch.float64, generator=g).requires_grad_()
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    lr, betas = 3e-3, (0.9, 0.999)
    opt = cls([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    q = p.detach().numpy().copy()
    m, v = np.zeros_like(q), np.zeros_like(q)
    worst = 0.0
    for t in range(1, 11):
        grad = torch.randn(3, 41, dtype=torch.float64, generator=g)
        p.grad = grad.clone()
        opt.step()
        q, m, v = adam_reference(q, grad, m, v, t, lr, betas[0], betas[1], eps, wd, decoupled)
        st = opt.state[p]
        for got, want in ((q, p), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            want = want.detach().numpy()
            worst = max(worst, float(np.linalg.norm(got - want) / np.linalg.norm(want)))
    print(f"worst relative L2 {worst:.3e}")
    assert worst <= 1e-12, worst


def test_adam_reference_conventions():
    """inv_ws scales the gradient before everything else; the first step of Adam moves every element by lr (eps -> 0);
    zero state and zero gradient stay zero; bad values are refused."""
    one = np.ones(4)
    p1, m1, v1 = adam_reference(one, 2 * one, 0 * one, 0 * one, 1, 0.5, 0.9, 0.999, 1e-30, 0.0, True, inv_ws=0.5)
    assert np.allclose(m1, 0.1 * one, rtol=1e-15) and np.allclose(v1, 0.001 * one, rtol=1e-12)
    assert np.allclose(p1, 0.5 * one, rtol=1e-12)
    z = np.zeros(3)
    for out in adam_reference(z, z, z, z, 1, 0.1, 0.9, 0.999, 1e-8, 0.05, True):
        assert np.array_equal(out, z)
    pa = adam_reference(one, z[:1], z[:1], z[:1], 1, 0.1, 0.9, 0.999, 1e-8, 0.05, True)[0]
    pl = adam_reference(one, z[:1], z[:1], z[:1], 1, 0.1, 0.9, 0.999, 1e-8, 0.05, False)[0]
    assert np.allclose(pa, 1 - 0.1 * 0.05) and np.allclose(pl, 1 - 0.1, rtol=1e-6)  # decoupled decay against L2
    for bad in (dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0), dict(wd=-1.0), dict(t=0)):
        kw = dict(t=1, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, decoupled=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            adam_reference(one, one, z[:1], z[:1], **kw)


# ---- FlatAdam on the CPU -----------------------------------------------------------------------------------------
def _flat_adam_worker(rank, ws, port, decoupled, overlap, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP
        torch.manual_seed(3)
        base = NetResDeep()
        a, b = copy.deepcopy(base), copy.deepcopy(base)
        ours = FlatBucketDDP(a, bucket_cap_mb=0.1)
        opt_a = FlatAdam(ours, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2, decoupled=decoupled,
                         overlap=overlap)
        theirs = torch.nn.parallel.DistributedDataParallel(b)
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        opt_b = cls(b.parameters(), lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2)
        for step in range(3):
            g = torch.Generator().manual_seed(1000 * step + rank)
            x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
            for model, opt in ((ours, opt_a), (theirs, opt_b)):
                loss = F.cross_entropy(model(x), y)
                opt.zero_grad()
                loss.backward()
                opt.step()
        assert opt_a.steps_taken() == 3
        # the bounds of test_flat_ddp's SGD comparison (the two all-reduces sum in different orders)
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert torch.allclose(pa, pb, atol=1e-5, rtol=1e-4), (n, float((pa - pb).abs().max()))
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


@pytest.mark.parametrize("decoupled,overlap", [(True, False), (True, True), (False, False)],
                         ids=["adamw", "adamw-overlap", "adam"])
def test_flat_adam_gloo_matches_torch(port, decoupled, overlap):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_flat_adam_worker, args=(r, 2, port, decoupled, overlap, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in res if r[1]]
    assert not bad, "\n".join(f"rank {r}:\n{e}" for r, e in bad)


# ---- flags -----------------------------------------------------------------------------------------------------------
def _parse(argv):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser()).parse_args(argv), "data/CIFAR-10/")


def test_flags_and_config_validation():
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig, check_optimizer_config
    cfg = _parse([])
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps) == ("sgd", 0.9, 0.999, 1e-8)
    assert not T.optimizer_active(cfg) and T.engine_optimizer(cfg, 10) is None
    cfg = _parse(["--optimizer", "adamw", "--weight-decay", "0.05", "--adam-beta2", "0.99", "--adam-eps", "1e-6",
                  "--epochs", "2"])
    assert T.optimizer_active(cfg)
    on = T.engine_optimizer(cfg, 5)
    assert (on.kind, tuple(on.betas), on.eps, on.weight_decay, on.momentum) == ("adamw", (0.9, 0.99), 1e-6, 0.05, 0.0)
    assert len(on.lr_table) == 10 and set(on.lr_table) == {1e-2}  # no schedule flag: a constant table
    assert T.engine_optimizer(_parse(["--optimizer", "adam"]), 5).kind == "adam"
    for argv in (["--optimizer", "adam", "--momentum", "0.9"], ["--optimizer", "adamw", "--momentum", "0.5"],
                 ["--optimizer", "adamw", "--adam-beta1", "1.0"], ["--optimizer", "adam", "--adam-beta2", "-0.1"],
                 ["--optimizer", "adamw", "--adam-eps", "0"], ["--optimizer", "adamw", "--adam-eps", "-1e-8"],
                 ["--optimizer", "adamw", "--weight-decay", "-0.1"]):
        with pytest.raises(SystemExit):
            _parse(argv)
    with pytest.raises(SystemExit):
        add_cli_args = T.add_cli_args(argparse.ArgumentParser())
        add_cli_args.parse_args(["--optimizer", "lamb"])
    assert _parse(["--momentum", "0.9", "--adam-beta1", "0.5"]).optimizer == "sgd"  # (unused values are not judged)
    check_optimizer_config(OptimizerConfig())
    check_optimizer_config(OptimizerConfig(kind="adamw", weight_decay=0.05))
    for bad in (dict(kind="adam", momentum=0.9), dict(kind="adamw", betas=(0.9, 1.0)), dict(kind="adam", eps=0.0),
                dict(kind="lamb"), dict(kind="adamw", betas=(0.9,)), dict(kind="adam", weight_decay=-1.0)):
        with pytest.raises(ValueError):
            check_optimizer_config(OptimizerConfig(**bad))


def test_generic_engines_build_adam_optimizers():
    """train_loop builds FlatAdam over a FlatBucketDDP and torch's Adam / AdamW over a plain module, with the flags'
    values; one CPU step of each gives the same parameters (FlatAdam's CPU fallback is torch's arithmetic)."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP
    cfg = T.TrainConfig(optimizer="adam", weight_decay=1e-3, adam_beta1=0.8, adam_beta2=0.95, adam_eps=1e-6, lr=3e-3)
    torch.manual_seed(2)
    plain = NetResDeep()
    flat = FlatBucketDDP(copy.deepcopy(plain))
    a, b = T.make_adam(plain, cfg), T.make_adam(flat, cfg)
    assert type(a) is torch.optim.Adam and isinstance(b, FlatAdam) and not b.decoupled
    assert a.defaults["betas"] == (0.8, 0.95) and a.defaults["eps"] == 1e-6 and a.defaults["weight_decay"] == 1e-3
    assert type(T.make_adam(NetResDeep(), T.TrainConfig(optimizer="adamw"))) is torch.optim.AdamW
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
        for model, opt in ((plain, a), (flat, b)):
            opt.zero_grad()
            F.cross_entropy(model(x), y).backward()
            opt.step()
    for (n, pa), pb in zip(plain.named_parameters(), flat.module.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6, rtol=1e-5), n


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


ADAMW = ["--synthetic", "256", "--optimizer", "adamw", "--weight-decay", "0.05", "--lr", "2e-3", "--lr-schedule",
         "cosine"]


def test_main_no_ddp_adamw_sidecar_and_resume(tmp_path, monkeypatch):
    """main_no_ddp.py --synthetic 256 --optimizer adamw --lr-schedule cosine on the CPU: the sidecar's keys; two epochs
    straight equal one epoch + --resume (checkpoint and both moments, bitwise); an SGD sidecar is refused by name."""
    from distributeddataparallel_cifar10_amd.train import optim_path
    a, b = str(tmp_path / "a" / "birds_vs_airplanes.pt"), str(tmp_path / "b" / "birds_vs_airplanes.pt")
    c = str(tmp_path / "c" / "birds_vs_airplanes.pt")
    _no_ddp_run(monkeypatch, 5, ADAMW + ["--epochs", "2", "--checkpoint-path", a])
    # (checkpoints are written at epoch 1, 10, 20, ...: the straight run's final state is what its module holds, so the
    # comparison runs both ways to epoch 2 and reads the resumed leg's state from a third file)
    straight = _no_ddp_run(monkeypatch, 5, ADAMW + ["--epochs", "2", "--no-checkpoint"])
    # first leg: the 2-epoch schedule stopped after epoch 1 (steps 1..4 run, the failure is raised at step 5)
    with pytest.raises(RuntimeError, match="injected failure"):
        _no_ddp_run(monkeypatch, 5, ADAMW + ["--epochs", "2", "--checkpoint-path", b, "--fail-at-step", "5"])
    assert sorted(os.listdir(tmp_path / "b")) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                                  "birds_vs_airplanes.pt.optim.pt"]
    side = torch.load(optim_path(b), weights_only=True)
    assert sorted(side) == ["exp_avg", "exp_avg_sq", "kind", "step"]
    assert side["step"] == 4 and side["kind"] == "adamw" and len(side["exp_avg"]) == len(side["exp_avg_sq"]) == 9
    assert all(float(v.abs().sum()) > 0 for v in side["exp_avg_sq"].values())
    assert len(torch.load(b, weights_only=True)) == 66

    seen = {}
    from distributeddataparallel_cifar10_amd import train as T
    real = T.make_adam

    def spy(model, cfg):
        seen["opt"] = real(model, cfg)
        return seen["opt"]
    monkeypatch.setattr(T, "make_adam", spy)
    resumed = _no_ddp_run(monkeypatch, 99, ADAMW + ["--epochs", "2", "--resume", b, "--no-checkpoint"])
    opt_b = seen["opt"]
    again = _no_ddp_run(monkeypatch, 5, ADAMW + ["--epochs", "2", "--no-checkpoint"])
    opt_a = seen["opt"]
    sa, sb = straight.state_dict(), resumed.state_dict()
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(sa[k], again.state_dict()[k]), k
    for pa, pb in zip(again.parameters(), resumed.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[pa][key], opt_b.state[pb][key]), key
        assert float(opt_a.state[pa]["step"]) == float(opt_b.state[pb]["step"]) == 8.0

    # an SGD sidecar (no "kind") under --optimizer adamw: the run ends with a message naming both kinds
    _no_ddp_run(monkeypatch, 5, ["--synthetic", "256", "--momentum", "0.9", "--epochs", "1", "--checkpoint-path", c])
    assert "kind" not in torch.load(optim_path(c), weights_only=True)
    with pytest.raises(SystemExit, match=r"--optimizer sgd.*--optimizer adamw"):
        _no_ddp_run(monkeypatch, 5, ADAMW + ["--epochs", "2", "--resume", c, "--no-checkpoint"])
    with pytest.raises(SystemExit, match=r"--optimizer adamw.*--optimizer sgd"):
        _no_ddp_run(monkeypatch, 5, ["--synthetic", "256", "--momentum", "0.9", "--epochs", "2", "--resume", b,
                                     "--no-checkpoint"])


def test_default_flags_write_todays_files(tmp_path, monkeypatch):
    """Default flags (SGD, no optimiser option): the checkpoint and its meta file, nothing else -- no sidecar."""
    p = str(tmp_path / "birds_vs_airplanes.pt")
    _no_ddp_run(monkeypatch, 5, ["--synthetic", "256", "--epochs", "1", "--checkpoint-path", p])
    assert sorted(os.listdir(tmp_path)) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json"]
