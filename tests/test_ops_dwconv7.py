"""Depthwise 7x7 convolution on the ops path (csrc/ops_dwconv7.hip), the parts that need no GPU: the integer inputs and
the float64 reference tests/test_ops_dwconv7_gpu.py uses, the launchers' shape rule, ``conv2d``'s routing and the
ConvNeXt model."""
import pytest
import torch
import torch.nn.functional as TF


def dwconv7_case(C, N, H, W):
    """(x, w, b, dy, y, dx, dw, db) in float64: x, dy in [-2, 2] NHWC, w in [-1, 1] [C, 1, 7, 7], b in [-2, 2] (|y| <=
    100: every product, fp32 partial sum and bf16 output of the kernels is exact), and torch's conv2d(groups=C) with
    its autograd gradients."""
    g = torch.Generator().manual_seed(7000 + 131 * C + 17 * H + W + N)
    x = torch.randint(-2, 3, (N, H, W, C), generator=g).double()
    dy = torch.randint(-2, 3, (N, H, W, C), generator=g).double()
    w = torch.randint(-1, 2, (C, 1, 7, 7), generator=g).double().requires_grad_()
    b = torch.randint(-2, 3, (C,), generator=g).double().requires_grad_()
    xn = x.permute(0, 3, 1, 2).requires_grad_()
    y = TF.conv2d(xn, w, b, padding=3, groups=C)
    y.backward(dy.permute(0, 3, 1, 2))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return x, w.detach(), b.detach(), dy, nhwc(y), nhwc(xn.grad), w.grad, b.grad


#                                  N, H,  W,  Cin, Cout, groups, K, stride, pad
@pytest.mark.parametrize("args,ok", [((1, 1, 1, 8, 8, 8, 7, 1, 3), True),
                                     ((1, 3, 64, 32, 32, 32, 7, 1, 3), True),      # the widest row
                                     ((2, 7, 7, 136, 136, 136, 7, 1, 3), True),
                                     ((1, 3, 65, 32, 32, 32, 7, 1, 3), False),     # W 65
                                     ((1, 5, 5, 12, 12, 12, 7, 1, 3), False),      # C % 8
                                     ((1, 5, 5, 16, 16, 16, 5, 1, 2), False),      # 5x5
                                     ((1, 5, 5, 16, 16, 16, 3, 1, 1), False),      # 3x3
                                     ((1, 5, 5, 16, 16, 16, 7, 2, 3), False),      # stride 2
                                     ((1, 5, 5, 16, 16, 16, 7, 1, 2), False),      # pad 2
                                     ((1, 5, 5, 16, 32, 16, 7, 1, 3), False),      # Cout != Cin
                                     ((1, 5, 5, 16, 16, 4, 7, 1, 3), False),       # groups != C
                                     ((2 ** 15, 64, 64, 16, 16, 16, 7, 1, 3), False)])  # 2^31 elements
def test_rule_boundaries(args, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    n, h, w, ci, co, groups, k, stride, pad = args
    assert (N.lib().dca_ops_dwconv7_rule(n, h, w, ci, co, groups, k, k, stride, pad) == 0) == ok
    if not ok:
        assert b"depthwise" in N.lib().dca_ops_last_error() and b"7x7" in N.lib().dca_ops_last_error()


@pytest.mark.parametrize("xshape,stride,pad,relu,match", [((1, 4, 65, 16), 1, 3, False, "7x7, pad 3, stride 1"),
                                                          ((1, 4, 4, 12), 1, 3, False, "7x7, pad 3, stride 1"),
                                                          ((1, 4, 4, 16), 2, 3, False, "7x7, pad 3, stride 1"),
                                                          ((1, 4, 4, 16), 1, 2, False, "7x7, pad 3, stride 1"),
                                                          ((1, 4, 4, 16), 1, 3, True, "no ReLU")])
def test_conv2d_refusals(xshape, stride, pad, relu, match):
    from distributeddataparallel_cifar10_amd.ops import conv2d
    c = xshape[-1]
    with pytest.raises(ValueError, match=match):
        conv2d(torch.zeros(xshape, dtype=torch.bfloat16), torch.zeros(c, 1, 7, 7), torch.zeros(c), stride=stride,
               pad=pad, relu=relu, groups=c)


@pytest.mark.parametrize("classes,params", [(1000, 28_589_128), (10, 27_827_818)])
def test_convnext_tiny(classes, params):
    from distributeddataparallel_cifar10_amd.models.convnext import convnext_tiny
    from distributeddataparallel_cifar10_amd.ops import OpsModel
    with torch.random.fork_rng(devices=[]):  # (the process's generator is left as it was found)
        net = convnext_tiny(num_classes=classes)
    assert sum(p.numel() for p in net.parameters()) == params
    dws = [b.dwconv for s in net.stages for b in s]
    assert [len(s) for s in net.stages] == [3, 3, 9, 3] and len(dws) == 18
    assert all(c.kernel_size == (7, 7) and c.padding == (3, 3) and c.stride == (1, 1) and c.bias is not None
               and c.groups == c.in_channels == c.out_channels for c in dws)
    assert OpsModel(net).kind == "convnext"
    with pytest.raises(ValueError, match="fp8 is not available for a ConvNeXt"):
        OpsModel(net, fp8=True)
