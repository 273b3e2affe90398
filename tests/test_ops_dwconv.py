"""Depthwise 3x3 convolution on the ops path (csrc/ops_dwconv.hip), the parts that need no GPU: the integer inputs and
the float64 reference tests/test_ops_dwconv_gpu.py uses (those of tests/test_ops_gconv.py at Cg = 1), the launchers'
shape rule, and the MobileNetV1 model."""
import pytest
import torch

from test_ops_gconv import gconv_inputs, gconv_ref


def dwconv_case(C, stride, N, H, W):
    """(x, w, dy, y, dx, dw) in float64: x, dy in [-4, 4] NHWC, w in [-2, 2] [C, 1, 3, 3] (every product, fp32 partial
    sum and bf16 output of the kernels is exact), and torch's conv2d(groups=C) with its autograd gradients."""
    x, w, dy = gconv_inputs(1, C, stride, N, H, W)
    return (x, w, dy) + gconv_ref(x, w, dy, stride, C)


#                                  N, H,  W,   Cin, Cout, groups, K, stride, pad
@pytest.mark.parametrize("args,ok", [((1, 3, 128, 32, 32, 32, 3, 1, 1), True),    # the widest row
                                     ((2, 5, 5, 8, 8, 8, 3, 1, 1), True),         # one chunk
                                     ((1, 9, 19, 72, 72, 72, 3, 2, 1), True),     # stride 2, odd H and W
                                     ((1, 3, 129, 32, 32, 32, 3, 1, 1), False),   # W 129
                                     ((1, 5, 5, 12, 12, 12, 3, 1, 1), False),     # C % 8
                                     ((1, 5, 5, 16, 16, 16, 5, 1, 2), False),     # 5x5
                                     ((1, 5, 5, 16, 16, 16, 3, 3, 1), False),     # stride 3
                                     ((1, 5, 5, 16, 32, 16, 3, 1, 1), False),     # Cin != Cout (a channel multiplier)
                                     ((1, 5, 5, 16, 16, 4, 3, 1, 1), False)])     # groups != C
def test_rule_boundaries(args, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    n, h, w, ci, co, groups, k, stride, pad = args
    assert (N.lib().dca_ops_dwconv_rule(n, h, w, ci, co, groups, k, k, stride, pad) == 0) == ok
    if not ok:
        assert b"rule" in N.lib().dca_ops_last_error() and b"depthwise" in N.lib().dca_ops_last_error()


@pytest.mark.parametrize("xshape,wshape,stride,pad", [((1, 4, 4, 16), (16, 1, 5, 5), 1, 2),
                                                      ((1, 4, 4, 12), (12, 1, 3, 3), 1, 1),
                                                      ((1, 4, 129, 16), (16, 1, 3, 3), 1, 1),
                                                      ((1, 4, 4, 16), (16, 1, 3, 3), 3, 1),
                                                      ((1, 4, 4, 16), (32, 1, 3, 3), 1, 1)])
def test_conv2d_outside_the_rule_raises(xshape, wshape, stride, pad):
    from distributeddataparallel_cifar10_amd.ops import conv2d
    with pytest.raises(ValueError, match="depthwise-convolution rule is 3x3, pad 1"):
        conv2d(torch.zeros(xshape, dtype=torch.bfloat16), torch.zeros(wshape), stride=stride, pad=pad,
               groups=xshape[-1])


def test_conv2d_depthwise_refuses_bias_and_relu():
    from distributeddataparallel_cifar10_amd.ops import conv2d
    x, w = torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16), torch.zeros(16, 1, 3, 3)
    with pytest.raises(ValueError, match="no bias and no ReLU"):
        conv2d(x, w, torch.zeros(16), stride=1, pad=1, groups=16)
    with pytest.raises(ValueError, match="no bias and no ReLU"):
        conv2d(x, w, stride=1, pad=1, relu=True, groups=16)


@pytest.mark.parametrize("classes,params", [(1000, 4_231_976), (10, 3_217_226)])
def test_mobilenet_parameters(classes, params):
    from distributeddataparallel_cifar10_amd.models.mobilenet import MobileNetV1
    with torch.random.fork_rng(devices=[]):  # (the process's generator is left as it was found)
        net = MobileNetV1(num_classes=classes)
    assert sum(p.numel() for p in net.parameters()) == params
    dws = [b.dw for b in net.blocks]
    assert len(dws) == 13 and all(c.groups == c.in_channels == c.out_channels for c in dws)
    assert [c.stride[0] for c in dws] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
