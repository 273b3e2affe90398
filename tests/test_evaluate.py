"""Eval-mode NetResDeep on the CPU tier: the torch evaluation path against stock PyTorch, the eval oracle, sharding over
ranks, the native entry's argument checks (no device needed) and the ``--eval`` / ``--eval-only`` flags."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
from distributeddataparallel_cifar10_amd.runtime import native
from distributeddataparallel_cifar10_amd.runtime.evaluate import (_DcaEvalArgs, eval_shard, evaluate_distributed,
                                                                  evaluate_netresdeep)
from distributeddataparallel_cifar10_amd.utils.oracle import normalize_u8, reference_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def _trained(steps=6, n=96, seed=3):
    """A NetResDeep a few SGD steps from its initialisation (running statistics moved), left in training mode."""
    torch.manual_seed(seed)
    model = NetResDeep()
    data, labels = synthetic_cifar(n, seed=seed, learnable=True)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    for s in range(steps):
        sel = slice(16 * (s % 4), 16 * (s % 4) + 16)
        opt.zero_grad()
        F.cross_entropy(model(normalize_u8(data[sel])), labels[sel]).backward()
        opt.step()
    return model, data, labels


@pytest.fixture(scope="module")
def trained():
    return _trained()


def test_cpu_evaluation_matches_stock_torch(trained):
    model, data, labels = trained
    state = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.training
    res = evaluate_netresdeep(model, data, labels, return_logits=True)
    assert model.training and all(m.training for m in model.modules())
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    model.eval()
    with torch.no_grad():
        want = model(normalize_u8(data))
    model.train()
    assert torch.equal(res.logits, want)
    assert res.count == len(data)
    assert res.correct == int((want.argmax(1) == labels).sum())
    assert torch.equal(res.pred.long(), want.argmax(1))
    ce = float(F.cross_entropy(want, labels, reduction="sum"))
    assert res.loss_sum == pytest.approx(ce, rel=1e-5)  # float64 sum of the fp32 per-image losses vs an fp32 sum
    assert res.accuracy == res.correct / res.count and res.mean_loss == res.loss_sum / res.count
    # a subset, in another order, chunked or not: the rows of the full run
    idx = [95, 0, 7, 7, 31]
    sub = evaluate_netresdeep(model, data, labels, indices=idx, return_logits=True)
    assert sub.count == 5  # (another batch size: the CPU convolution may pick another algorithm, hence not bitwise)
    torch.testing.assert_close(sub.logits, want[idx], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        evaluate_netresdeep(model, data, labels, indices=[0, len(data)])
    with pytest.raises(ValueError):
        evaluate_netresdeep(model, data, labels, indices=[-1])


def test_reference_eval_is_the_module_in_eval_mode(trained):
    model, data, _ = trained
    model.eval()
    with torch.no_grad():
        want = model(normalize_u8(data[:40]))
    model.train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    got = reference_eval(model, data[:40])
    assert torch.equal(got, want)  # bitwise with both switches off
    assert model.training and all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    # the rounding switches change the result, a little
    rounded = reference_eval(model, data[:40], bf16_operands=True, fc1_bf16=True)
    rel = float((rounded - want).norm() / want.norm())
    assert 0 < rel < 5e-2


@pytest.mark.parametrize("ws", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 7, 10000])
def test_eval_shard_partitions_the_range(n, ws):
    parts = [eval_shard(n, ws, r) for r in range(ws)]
    assert sorted(np.concatenate(parts).tolist()) == list(range(n))  # every image exactly once, none padded
    assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    with pytest.raises(ValueError):
        eval_shard(n, ws, ws)


def _case_distributed(rank, ws):
    model, data, labels = _trained()
    if rank == 1:  # a rank's own running statistics between two steps: rank 0's are the ones evaluated
        with torch.no_grad():
            model.resblocks[0].batch_norm.running_mean += 0.25
    own = model.resblocks[0].batch_norm.running_mean.clone()
    got = evaluate_distributed(model, data[:37], labels[:37])
    ref_model, _, _ = _trained()
    want = evaluate_netresdeep(ref_model, data[:37], labels[:37])
    assert (got.correct, got.count) == (want.correct, want.count) == (want.correct, 37)
    assert got.loss_sum == pytest.approx(want.loss_sum, rel=1e-5)  # two shards: other batch sizes than one pass
    assert got.count == 37 and len(got.pred) == len(eval_shard(37, ws, rank))
    assert torch.equal(model.resblocks[0].batch_norm.running_mean, own)  # the module's buffers are not touched


def test_evaluate_distributed_two_gloo_ranks(port):
    from test_flat_ddp import _spawn
    _spawn(_case_distributed, port, ws=2)


def test_evaluate_distributed_without_a_group(trained):
    model, data, labels = trained
    a, b = evaluate_distributed(model, data, labels), evaluate_netresdeep(model, data, labels)
    assert (a.correct, a.count, a.loss_sum) == (b.correct, b.count, b.loss_sum)


def test_native_eval_entry_validates_before_any_launch():
    """dca_eval_netresdeep checks its arguments on the host, before any device call: on a machine without a GPU a bad
    call returns -1 with a message (a launch attempt would fail with a HIP error instead)."""
    lib = native.load()
    assert lib.dca_abi_version() == native.ABI_VERSION == 10
    assert hasattr(lib, "dca_eval_netresdeep")
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def args(**over):
        a = _DcaEvalArgs(*([p] * 11), 1e-5, p, p, 4, p, 4, 1, 0, p, p, p)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def rejected(a, word):
        assert lib.dca_eval_netresdeep(ctypes.byref(a), None) == -1
        assert word in native.last_error(), native.last_error()

    for name in ("conv1_w", "conv_w", "bn_rv", "fc1_w", "fc2_b", "data", "labels", "indices", "pred", "loss"):
        rejected(args(**{name: None}), name)
    rejected(args(n=0), "positive")
    rejected(args(n=-3), "positive")
    rejected(args(n_data=0), "positive")
    rejected(args(fc1_w=p + 4), "misaligned")
    rejected(args(conv_w=p + 2), "misaligned")
    rejected(args(max_workgroups=-1), "negative")
    assert lib.dca_eval_netresdeep(None, None) == -1


def _run(args, timeout=400):
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=ENV, capture_output=True, text=True, timeout=timeout)


TEST_LINE = r"Epoch 1, Test accuracy (\d\.\d{4}), Test loss (\d+\.\d+(e-?\d+)?)"


def test_cli_eval_flag(tmp_path):
    mj = tmp_path / "m.json"
    base = ["main_no_ddp.py", "--synthetic", "256", "--epochs", "1", "--max-steps", "4"]
    r = _run(base + ["--eval", "64", "--metrics-json", str(mj)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    hits = [re.fullmatch(TEST_LINE, ln) for ln in lines if "Test accuracy" in ln]
    assert len(hits) == 1 and hits[0], lines
    assert lines.index(hits[0].group(0)) == lines.index(next(ln for ln in lines if "Training loss" in ln)) + 1
    recs = [json.loads(ln) for ln in mj.read_text().splitlines()]
    ep = [x for x in recs if x.get("epoch") == 1][0]
    assert ep["eval_images"] == 64 and 0.0 <= ep["eval_accuracy"] <= 1.0 and ep["eval_loss"] > 0
    assert f"{ep['eval_accuracy']:.4f}" == hits[0].group(1) and float(hits[0].group(2)) == ep["eval_loss"]
    # without the flag: the lines of before, and no eval fields
    mj2 = tmp_path / "m2.json"
    r2 = _run(base + ["--metrics-json", str(mj2)])
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "Test" not in r2.stdout and len(r2.stdout.strip().splitlines()) == len(lines) - 1
    assert not any(k.startswith("eval") for ln in mj2.read_text().splitlines() for k in json.loads(ln))


def test_cli_eval_only(tmp_path, port):
    ck = tmp_path / "birds_vs_airplanes.pt"
    common = ["--synthetic", "256", "--eval", "64"]
    r = _run(["main.py", "--backend", "gloo", "--world-size", "1", "--epochs", "1", "--max-steps", "4", "--engine",
              "torch", "--checkpoint-path", str(ck), "--port", str(port)] + common)
    assert r.returncode == 0, r.stderr[-3000:]
    m = re.search(TEST_LINE, r.stdout)
    assert m, r.stdout
    before = ck.read_bytes()
    for entry in (["main_no_ddp.py"], ["main.py", "--backend", "gloo", "--world-size", "1", "--port", str(port)]):
        e = _run(entry + ["--eval-only", "--resume", str(ck)] + common)
        assert e.returncode == 0, e.stderr[-3000:]
        m2 = re.search(r"^Test accuracy (\d\.\d{4}), Test loss (\S+)$", e.stdout, re.M)
        assert m2 and m2.group(1) == m.group(1) and float(m2.group(2)) == pytest.approx(float(m.group(2)), rel=1e-6)
        assert "Training loss" not in e.stdout and "training time" not in e.stdout
    assert ck.read_bytes() == before and sorted(os.listdir(tmp_path)) == sorted(
        ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json"])
    bad = _run(["main_no_ddp.py", "--eval-only"] + common)
    assert bad.returncode != 0 and "--eval-only requires --resume" in bad.stderr
