"""Squeeze-and-excitation on the ops path (csrc/ops_se.hip), the parts that need no GPU: the launchers' shape rule, the
SE models, the order an ``SELink`` enforces, and the float64 reference tests/test_ops_se_gpu.py uses."""
import pytest
import torch


def se_ref(u, z, idt, dout, ds, out=None):
    """The four kernels in float64 from [N, H, W, C] u, idt, dout and [N, C] z, ds: (s, out, didt, dz, du).  ``out``:
    take the ReLU mask from this output (the tensor the backward kernels read) instead of the reference's own."""
    u, z, idt, dout, ds = (t.double() for t in (u, z, idt, dout, ds))
    p = u.shape[1] * u.shape[2]
    g = (1.0 / (1.0 + torch.exp(-z)))[:, None, None, :]
    out_ref = torch.relu(u * g + idt)
    didt = dout * ((out_ref if out is None else out.double()) > 0)
    dz = (didt * u).sum((1, 2)) * g[:, 0, 0] * (1.0 - g[:, 0, 0])
    return u.mean((1, 2)), out_ref, didt, dz, didt * g + ds[:, None, None, :] / p


@pytest.mark.parametrize("shape,ok", [((1, 1, 1, 8), True), ((2, 7, 7, 136), True), ((1, 1, 1, 12), False),
                                      ((1, 0, 1, 8), False), ((0, 1, 1, 8), False), ((4, 1 << 13, 1 << 13, 8), False),
                                      ((4, 1 << 13, (1 << 13) - 1, 8), True)])  # 2^31 elements; the largest below
def test_rule_boundaries(shape, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    assert (N.lib().dca_ops_se_rule(*shape) == 0) == ok
    if not ok:
        assert b"squeeze-and-excitation rule is" in N.lib().dca_ops_last_error()


@pytest.mark.parametrize("name,params", [("se_resnext50_32x4d", 27_559_896), ("se_resnet50", 28_088_024)])
def test_se_model_parameters(name, params):
    from distributeddataparallel_cifar10_amd.models import resnet50 as R
    with torch.random.fork_rng(devices=[]):  # (the process's generator is left as it was found)
        net, plain = getattr(R, name)(), getattr(R, name[3:])()
    se = sum(2 * c * (c // 16) + c + c // 16 for c, k in ((256, 3), (512, 4), (1024, 6), (2048, 3)) for _ in range(k))
    assert se == 2_530_992
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in plain.parameters()) + se == params
    blocks = [m for m in net.modules() if isinstance(m, R.Bottleneck)]
    assert len(blocks) == 16 and all(b.se.fc1.in_features == b.se.fc2.out_features == b.bn3.num_features and
                                     b.se.fc1.out_features == b.bn3.num_features // 16 for b in blocks)


def test_no_se_leaves_the_model_as_it_was():
    from distributeddataparallel_cifar10_amd.models.resnet50 import ResNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        a = ResNet([1, 1, 1, 1], num_classes=10)
        torch.manual_seed(0)
        b, draw = ResNet([1, 1, 1, 1], num_classes=10, se_reduction=0), torch.rand(1)
        torch.manual_seed(0)
        ResNet([1, 1, 1, 1], num_classes=10)
        assert torch.equal(draw, torch.rand(1))  # no extra RNG draw
        se = ResNet([1, 1, 1, 1], num_classes=10, se_reduction=16)
    assert list(a.state_dict()) == list(b.state_dict()) and not any(".se." in k for k in b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    extra = sorted(set(se.state_dict()) - set(a.state_dict()))
    assert extra == sorted(f"layer{i}.0.se.{fc}.{p}" for i in (1, 2, 3, 4) for fc in ("fc1", "fc2")
                           for p in ("weight", "bias"))


def test_link_order_and_fp8_refusal():
    from distributeddataparallel_cifar10_amd.models.resnet50 import ResNet
    from distributeddataparallel_cifar10_amd.ops import OpsModel, SELink, se_scale, se_squeeze
    u, z = torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16), torch.zeros(1, 8)
    with pytest.raises(RuntimeError, match="se_scale came when se_squeeze was due"):
        se_scale(u, z, u, SELink())
    used = SELink()
    used.advance(0)
    with pytest.raises(RuntimeError, match="se_squeeze came when se_scale was due"):
        se_squeeze(u, used)
    with pytest.raises(ValueError, match="squeeze-and-excitation rule is"):
        se_squeeze(torch.zeros(1, 2, 2, 12, dtype=torch.bfloat16), SELink())
    with torch.random.fork_rng(devices=[]):
        net = ResNet([1, 1, 1, 1], num_classes=10, se_reduction=16)
    with pytest.raises(ValueError, match="fp8 is not available for a squeeze-and-excitation model"):
        OpsModel(net, fp8=True)
