"""The training application's state plumbing (CPU): optimiser state out of and into every optimiser family through the
real sidecar writer, the one atomic writer, and the flag -> ``TrainConfig`` table."""
import argparse
import copy
import os

import pytest
import torch
import torch.nn as nn

from distributeddataparallel_cifar10_amd import train as T
from distributeddataparallel_cifar10_amd.backends import GenericBackend
from distributeddataparallel_cifar10_amd.data.cifar import normalize_u8
from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD
from distributeddataparallel_cifar10_amd.runtime.engine import optimizer_state_kind
from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint, unwrap
from distributeddataparallel_cifar10_amd.utils.ema import ModelEma, ema_path, save_ema_state

ADAM = dict(betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
# name -> (sidecar kind, wraps the module in FlatBucketDDP, optimiser factory)
FAMILIES = {
    "torch-sgd": ("sgd", False, lambda m: torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)),
    "flat-sgd": ("sgd", True, lambda m: FlatSGD(m, 0.05, momentum=0.9)),
    "torch-adamw": ("adamw", False, lambda m: torch.optim.AdamW(m.parameters(), lr=1e-2, **ADAM)),
    "flat-adam": ("adamw", True, lambda m: FlatAdam(m, 1e-2, **ADAM)),
}
TWIN = {"torch-sgd": "flat-sgd", "flat-sgd": "torch-sgd", "torch-adamw": "flat-adam", "flat-adam": "torch-adamw"}


@pytest.fixture(scope="module")
def batches():
    data, labels = synthetic_cifar(16, seed=0)
    return [(normalize_u8(data[i:i + 8]), labels[i:i + 8].long()) for i in (0, 8)]


def make(family: str, module: nn.Module, cfg=None):
    """(model as train_loop takes it, its backend) for `family` around `module`."""
    kind, flat, factory = FAMILIES[family]
    model = FlatBucketDDP(module) if flat else module
    return model, GenericBackend(model, factory(model), cfg or T.TrainConfig(optimizer=kind), 0, None)


def step(model, backend, batch) -> None:
    imgs, labels = batch
    loss = backend.loss_fn(model(imgs).float(), labels)
    backend.optimizer.zero_grad()
    loss.backward()
    backend.optimizer.step()


def fresh_copy(model) -> nn.Module:
    """A new NetResDeep holding `model`'s parameters and buffers as they are now."""
    twin = NetResDeep()
    twin.load_state_dict(copy.deepcopy(unwrap(model).state_dict()))
    return twin


def flat_state(backend) -> dict:
    """{"<entry>/<parameter name>": tensor} of the backend's optimiser state (its other entries dropped)."""
    return {f"{key}/{name}": t for key, value in backend.optimizer_state().items()
            if key in ("momentum_buffer", "exp_avg", "exp_avg_sq") for name, t in value.items()}


def steps_taken(backend):
    opt = backend.optimizer
    if isinstance(opt, FlatAdam):
        return opt.steps_taken()
    steps = {int(st["step"]) for st in opt.state.values() if "step" in st}
    assert len(steps) <= 1
    return steps.pop() if steps else None  # (SGD keeps no count: the sidecar's "step" is the schedule position)


def assert_same(a: dict, b: dict) -> None:
    assert sorted(a) == sorted(b)  # by name
    for k in a:  # bitwise: the bytes, so that a zero's sign counts
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(_bytes(a[k]), _bytes(b[k])), k


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_round_trip_through_the_sidecar(family, batches, tmp_path):
    """Two steps; the state through save_optimizer_state and torch.load(weights_only=True) into a fresh optimiser on a
    copy of the model: read back bitwise, the same step count, and a third step bitwise equal on both."""
    kind = FAMILIES[family][0]
    torch.manual_seed(3)
    model, backend = make(family, NetResDeep())
    for b in batches:
        step(model, backend, b)
    ckpt = str(tmp_path / "run" / "birds_vs_airplanes.pt")
    T.save_optimizer_state(backend, ckpt, 0, 2)
    written = torch.load(T.optim_path(ckpt), weights_only=True)
    assert written["step"] == 2 and optimizer_state_kind(written) == kind
    assert len(flat_state(backend)) == (9 if kind == "sgd" else 18)

    model2, backend2 = make(family, fresh_copy(model))
    assert T.load_optimizer_state(backend2, ckpt, 2, kind)
    assert_same(flat_state(backend2), flat_state(backend))
    assert_same(flat_state(backend2), {f"{k}/{n}": t for k, v in written.items() if isinstance(v, dict)
                                       for n, t in v.items()})
    assert steps_taken(backend2) == steps_taken(backend)
    assert steps_taken(backend) == (None if kind == "sgd" else 2)

    step(model, backend, batches[0])
    step(model2, backend2, batches[0])
    assert_same(dict(unwrap(model2).state_dict()), dict(unwrap(model).state_dict()))
    assert_same(flat_state(backend2), flat_state(backend))
    assert steps_taken(backend2) == steps_taken(backend)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_sidecar_loads_into_the_other_family(family, batches, tmp_path):
    """A sidecar written from one family loads into its twin of the same kind (a --engine torch checkpoint resumes on
    --engine ops and the reverse): read back by parameter name, bitwise."""
    kind = FAMILIES[family][0]
    torch.manual_seed(4)
    model, backend = make(family, NetResDeep())
    for b in batches:
        step(model, backend, b)
    ckpt = str(tmp_path / "birds_vs_airplanes.pt")
    T.save_optimizer_state(backend, ckpt, 0, 2)
    _, twin = make(TWIN[family], fresh_copy(model))
    assert T.load_optimizer_state(twin, ckpt, 2, kind)
    assert_same(flat_state(twin), flat_state(backend))
    assert steps_taken(twin) == steps_taken(backend)


def test_state_before_the_first_step(tmp_path):
    for family in ("torch-sgd", "flat-sgd"):
        model, backend = make(family, NetResDeep())
        assert backend.optimizer_state() == {"momentum_buffer": {}}
        ckpt = str(tmp_path / family / "birds_vs_airplanes.pt")
        T.save_optimizer_state(backend, ckpt, 0, 0)
        assert torch.load(T.optim_path(ckpt), weights_only=True) == {"step": 0, "momentum_buffer": {}}
        assert T.load_optimizer_state(backend, ckpt, 0, "sgd")  # a no-op
        assert backend.optimizer_state() == {"momentum_buffer": {}} and not backend.optimizer.state
    _, backend = make("flat-adam", NetResDeep())
    state = backend.optimizer_state()
    assert list(state) == ["kind", "exp_avg", "exp_avg_sq"] and state["kind"] == "adamw"
    for key in ("exp_avg", "exp_avg_sq"):
        assert len(state[key]) == 9 and all(not t.any() for t in state[key].values())
    _, backend = make("torch-adamw", NetResDeep())
    assert backend.optimizer_state() == {"kind": "adamw", "exp_avg": {}, "exp_avg_sq": {}}


def test_one_writer_for_the_three_files(batches, tmp_path):
    """Checkpoint (+ meta), optimiser sidecar and .ema.pt: no tmp file is left behind, the two state_dict files hold
    66 keys over 12 storages, and a rank other than 0 writes nothing."""
    torch.manual_seed(5)
    model, backend = make("flat-sgd", NetResDeep())
    ema = ModelEma(model, 0.9)
    step(model, backend, batches[0])
    ema.update(0)
    ckpt = str(tmp_path / "out" / "birds_vs_airplanes.pt")
    quiet = str(tmp_path / "rank1" / "birds_vs_airplanes.pt")
    for path, rank in ((quiet, 1), (ckpt, 0)):
        for write in (lambda: T.save_optimizer_state(backend, path, rank, 1),
                      lambda: save_checkpoint(model, path, rank, meta={"epoch": 1, "step": 1}),
                      lambda: save_ema_state(ema.state_dict(), path, rank)):
            write()
            assert rank or not [n for n in os.listdir(os.path.dirname(path)) if ".tmp." in n]
        if rank:
            assert not os.path.exists(os.path.dirname(path))
        else:
            assert sorted(os.listdir(os.path.dirname(path))) == [
                "birds_vs_airplanes.pt", "birds_vs_airplanes.pt.ema.pt", "birds_vs_airplanes.pt.meta.json",
                "birds_vs_airplanes.pt.optim.pt"]  # (so no *.tmp.* either)
    for path in (ckpt, ema_path(ckpt)):
        sd = torch.load(path, weights_only=True)
        assert len(sd) == 66 and len({t.untyped_storage().data_ptr() for t in sd.values()}) == 12, path


# ---- the flag table ----------------------------------------------------------------------------------------------
# flags whose TrainConfig field has another name, and the flags that set two fields by design or none
FIELDS_OF = {"data_root": {"data_path"}, "timeout": {"timeout_s"}, "no_checkpoint": {"checkpoint"},
             "augment_no_flip": {"augment_flip"}, "synthetic_learnable": {"synthetic_learnable", "synthetic"},
             "eval_only": {"eval_only", "eval"}, "world_size": set()}  # (--world-size is the launcher's, not the run's)


def _other_value(action):
    if action.nargs == 0:
        return []
    if action.choices:
        return [next(c for c in action.choices if c != action.default)]
    if action.type in (int, float):
        return [str((action.default or 0) + (3 if action.type is int else 0.25))]
    return ["elsewhere"]


def test_every_flag_sets_exactly_its_field():
    ap = T.add_cli_args(argparse.ArgumentParser())
    base_argv = ["--resume", "ckpt.pt"]  # (--eval-only needs one)
    base = T.config_from_args(ap.parse_args(base_argv), "data/CIFAR-10/")
    names = [f for f in T.TrainConfig.__dataclass_fields__]
    for action in (a for a in ap._actions if a.dest != "help"):
        cfg = T.config_from_args(ap.parse_args(base_argv + [action.option_strings[0]] + _other_value(action)),
                                 "data/CIFAR-10/")
        changed = {f for f in names if getattr(cfg, f) != getattr(base, f)}
        assert changed == FIELDS_OF.get(action.dest, {action.dest}), (action.dest, changed)
    assert T.config_from_args(argparse.Namespace(resume=None), "d") == T.TrainConfig(data_path="d")  # a bare namespace
