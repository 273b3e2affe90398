"""Grouped 3x3 convolution on the ops path (csrc/ops_gconv.hip), the parts that need no GPU: the float64 reference and the
integer input generator tests/test_ops_gconv_gpu.py uses, the ResNeXt-50 model, and the launchers' shape rule."""
import pytest
import torch
import torch.nn.functional as TF


def gconv_inputs(Cg, C, stride, N, H, W, seed=0):
    """(x, w, dy) as float64 NHWC / torch-layout tensors of small integers (x, dy in [-4, 4], w in [-2, 2]): every
    product and every fp32 partial sum of the kernels is exact."""
    g = torch.Generator().manual_seed(seed + 131 * Cg + C + 7 * stride + H)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randint(-4, 5, (N, H, W, C), generator=g).double()
    w = torch.randint(-2, 3, (C, Cg, 3, 3), generator=g).double()
    dy = torch.randint(-4, 5, (N, Ho, Wo, C), generator=g).double()
    return x, w, dy


def gconv_ref(x, w, dy, stride, groups):
    """(y, dx, dw) of torch's float64 grouped conv and its autograd gradients; NHWC in, NHWC out."""
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_()
    wn = w.clone().requires_grad_()
    y = TF.conv2d(xn, wn, stride=stride, padding=1, groups=groups)
    y.backward(dy.permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), xn.grad.permute(0, 2, 3, 1).contiguous(), wn.grad


def test_resnext50_parameters_and_resnet50_unchanged():
    from distributeddataparallel_cifar10_amd.models.resnet50 import ResNet, resnet50, resnext50_32x4d
    assert sum(p.numel() for p in resnext50_32x4d().parameters()) == 25_028_904
    with torch.random.fork_rng(devices=[]):  # (the process's generator is left as it was found)
        torch.manual_seed(5)
        a = resnet50(num_classes=10)
        assert sum(p.numel() for p in resnet50().parameters()) == 25_557_032
        torch.manual_seed(5)
        b = ResNet([3, 4, 6, 3], 10, groups=1, width_per_group=64)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    assert a.layer1[0].conv2.weight.shape == (64, 64, 3, 3) and a.layer1[0].conv2.groups == 1


#                                  N, H,  W,  Cin, Cout, groups, K, stride, pad
@pytest.mark.parametrize("args,ok", [((2, 5, 19, 48, 48, 12, 3, 1, 1), True), ((1, 7, 64, 96, 96, 3, 3, 2, 1), True),
                                     ((1, 7, 64, 32, 32, 16, 3, 1, 1), False),   # Cg 2
                                     ((1, 7, 64, 128, 128, 2, 3, 1, 1), False),  # Cg 64
                                     ((1, 7, 65, 48, 48, 12, 3, 1, 1), False),   # W 65
                                     ((1, 7, 17, 24, 24, 6, 3, 1, 1), False),    # C % 16
                                     ((1, 7, 17, 48, 96, 12, 3, 1, 1), False),   # Cin != Cout
                                     ((1, 7, 17, 48, 48, 12, 5, 1, 2), False),   # 5x5
                                     ((1, 7, 17, 48, 48, 12, 3, 3, 1), False),   # stride 3
                                     ((1, 7, 17, 48, 48, 1, 3, 1, 1), False)])   # not grouped
def test_rule_boundaries(args, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    n, h, w, ci, co, groups, k, stride, pad = args
    assert (N.lib().dca_ops_gconv_rule(n, h, w, ci, co, groups, k, k, stride, pad) == 0) == ok
    if not ok:
        assert b"rule" in N.lib().dca_ops_last_error()


@pytest.mark.parametrize("xshape,wshape,groups,stride,pad", [((1, 4, 4, 32), (32, 2, 3, 3), 16, 1, 1),
                                                             ((1, 4, 70, 32), (32, 4, 3, 3), 8, 1, 1),
                                                             ((1, 4, 4, 32), (32, 4, 5, 5), 8, 1, 2),
                                                             ((1, 4, 4, 32), (64, 4, 3, 3), 8, 1, 1)])
def test_conv2d_outside_the_rule_raises(xshape, wshape, groups, stride, pad):
    from distributeddataparallel_cifar10_amd.ops import conv2d, gconv_ok
    assert not gconv_ok(xshape, wshape, stride, pad, groups)
    with pytest.raises(ValueError, match="rule is 3x3, pad 1"):
        conv2d(torch.zeros(xshape, dtype=torch.bfloat16), torch.zeros(wshape), stride=stride, pad=pad, groups=groups)
