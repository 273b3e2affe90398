"""The training application's state plumbing on an MI355X: the optimiser state of ``FlatSGD`` / ``FlatAdam`` on the
device (the HIP kernels' "buffer initialised" flag after a load; the device step state with its running beta products)
through the real sidecar writer, and the fused engine's state into ``FlatAdam`` and back.  NetResDeep through
``OpsModel`` + ``FlatBucketDDP``, batch 8, 16 synthetic images."""
import pytest
import torch

from test_train_state import FAMILIES, assert_same, flat_state, fresh_copy, step, steps_taken

pytestmark = pytest.mark.gpu


def _make(family, module, dev):
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.backends import GenericBackend
    from distributeddataparallel_cifar10_amd.ops.models import OpsModel
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatBucketDDP
    kind, _, factory = FAMILIES[family]
    model = FlatBucketDDP(OpsModel(module.to(dev)))
    return model, GenericBackend(model, factory(model), T.TrainConfig(optimizer=kind, engine="ops"), 0, None)


def _batches(dev):
    from distributeddataparallel_cifar10_amd.data.cifar import normalize_u8
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    data, labels = synthetic_cifar(16, seed=0)
    data, labels = data.to(dev), labels.to(dev)
    return [(normalize_u8(data[i:i + 8]), labels[i:i + 8].long()) for i in (0, 8)]


@pytest.mark.parametrize("family", ["flat-sgd", "flat-adam"])
def test_round_trip_on_the_device(gpu, family, tmp_path):
    """tests/test_train_state.py test_round_trip_through_the_sidecar with the HIP kernels: after the load the SGD
    kernel must not treat the buffer as uninitialised, and the Adam kernel continues with the bias of step 3."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    kind, batches = FAMILIES[family][0], _batches(gpu)
    torch.manual_seed(3)
    model, backend = _make(family, NetResDeep(), gpu)
    for b in batches:
        step(model, backend, b)
    ckpt = str(tmp_path / "birds_vs_airplanes.pt")
    T.save_optimizer_state(backend, ckpt, 0, 2)
    written = torch.load(T.optim_path(ckpt), weights_only=True)
    model2, backend2 = _make(family, fresh_copy(model), gpu)
    assert T.load_optimizer_state(backend2, ckpt, 2, kind)
    assert_same(flat_state(backend2), flat_state(backend))
    assert_same(flat_state(backend2), {f"{k}/{n}": t for k, v in written.items() if isinstance(v, dict)
                                       for n, t in v.items()})
    assert all(float(t.abs().sum()) > 0 for t in flat_state(backend).values())
    if kind != "sgd":
        assert steps_taken(backend2) == steps_taken(backend) == 2
    step(model, backend, batches[0])
    step(model2, backend2, batches[0])
    torch.cuda.synchronize()
    from distributeddataparallel_cifar10_amd.utils.checkpoint import unwrap
    assert_same(dict(unwrap(model2).state_dict()), dict(unwrap(model).state_dict()))
    assert_same(flat_state(backend2), flat_state(backend))
    assert steps_taken(backend2) == steps_taken(backend)


def test_fused_engine_state_into_flat_adam_and_back(gpu, tmp_path):
    """The fused engine's optimiser state (its sidecar, ``"engine"`` entry included) loads into a ``FlatAdam`` -- a
    ``--engine fused`` checkpoint resumes on ``--engine ops`` -- and the ``FlatAdam``'s sidecar back into the engine:
    read back by parameter name, bitwise."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.backends import FusedBackend
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel.ddp import FusedDDPTrainer
    cfg = T.TrainConfig(optimizer="adamw", weight_decay=0.05, lr=1e-2, batch_size=8, epochs=2, dtype="bf16")
    data, labels = synthetic_cifar(16, seed=0)
    loader = DeviceLoader(data, labels, batch_size=8, device=gpu, sampler="sequential")
    torch.manual_seed(3)
    trainer = FusedDDPTrainer(NetResDeep().to(gpu), loader.data, loader.labels, batch_max=8, lr=cfg.lr, dtype="bf16",
                              max_indices=16, optimizer=T.engine_optimizer(cfg, len(loader)))
    try:
        fused = FusedBackend(trainer, cfg, 0, T.lr_table_for(cfg, len(loader)))
        assert fused.run_epoch(loader, 2, 0)[1] == 2
        want = {k: t.clone() for k, t in flat_state(fused).items()}
        assert len(want) == 18 and all(float(t.abs().sum()) > 0 for t in want.values())
        a, b = str(tmp_path / "fused.pt"), str(tmp_path / "flat.pt")
        T.save_optimizer_state(fused, a, 0, 2)
        assert "engine" in torch.load(T.optim_path(a), weights_only=True)
        _, flat = _make("flat-adam", NetResDeep(), gpu)
        assert T.load_optimizer_state(flat, a, 2, "adamw")
        assert_same(flat_state(flat), want)
        assert steps_taken(flat) == 2
        T.save_optimizer_state(flat, b, 0, 2)
        fused.run_epoch(loader, 1, 2)  # the engine's state moves on ...
        assert trainer.engine.optimizer_step() == 3
        assert T.load_optimizer_state(fused, b, 2, "adamw")  # ... and comes back from the FlatAdam's file
        assert_same(flat_state(fused), want)
        assert trainer.engine.optimizer_step() == 2
    finally:
        trainer.close()
