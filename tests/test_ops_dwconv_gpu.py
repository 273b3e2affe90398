"""The depthwise 3x3 kernels (csrc/ops_dwconv.hip) on an MI355X against torch's float64 conv2d(groups=C)
(tests/test_ops_dwconv.py): integer inputs make every fp32 sum exact, so forward, input gradient and weight gradient are
compared bit for bit."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as TF

from test_ops_dwconv import dwconv_case

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# (C, N, H, W): one chunk and one pixel; two images, a 1 x 1 stride-2 output; a full 64-channel slab plus a ragged one,
# more rows than ring slots, odd sizes, strips crossing an image boundary; two columns per thread; the widest row; the
# widest odd row; the 128-channel slab of the narrow rows plus a ragged one
SHAPES = [(8, 1, 1, 1), (8, 2, 2, 2), (72, 2, 9, 19), (40, 1, 5, 65), (32, 1, 3, 128), (16, 1, 4, 127), (136, 1, 5, 13)]
CASES = [(c, s, n, h, w) for s in (1, 2) for c, n, h, w in SHAPES]
NPARTS = 4  # statistics rows / weight-gradient slabs: fewer than the units of some cases, more than those of others


@functools.lru_cache(maxsize=None)
def _case(c, s, n, h, w):  # inputs and float64 reference, computed once per case and never modified
    return dwconv_case(c, s, n, h, w)


@pytest.mark.parametrize("c,s,n,h,w", CASES)
def test_forward_and_bn_partial_sums(gpu, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    x, wt, _, y_ref, _, _ = _case(c, s, n, h, w)
    xd, wd = x.to(BF16).to(gpu), wt.float().to(gpu)
    shift = (0.25 * (torch.arange(c) % 4 + 1) * (1 - 2 * (torch.arange(c) % 2))).float()  # dyadic, non-zero
    outs = []
    for _ in range(2):
        y = torch.full(y_ref.shape, float("nan"), dtype=BF16, device=gpu)
        part = torch.full((NPARTS, c, 2), float("nan"), device=gpu)
        N.check(N.lib().dca_ops_dwconv_fwd(N.ptr(xd), N.ptr(wd), N.ptr(y), N.ptr(part), N.ptr(shift.to(gpu)), NPARTS,
                                           n, h, w, c, c, s, N.stream(gpu)), "dwconv_fwd")
        outs.append((y.cpu(), part.cpu()))
    want = y_ref.to(BF16)
    assert torch.equal(outs[0][0], want)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    v = want.double().view(-1, c) - shift.double()
    got = outs[0][1].double().sum(0)  # [c, 2]
    tol = NPARTS * 2.0 ** -24  # one fp32 rounding per row summed (tests/test_ops_gconv_gpu.py)
    assert ((got[:, 0] - v.sum(0)).abs() <= tol * v.abs().sum(0)).all()
    assert ((got[:, 1] - (v * v).sum(0)).abs() <= tol * (v * v).sum(0)).all()


@pytest.mark.parametrize("c,s,n,h,w", CASES)
def test_input_gradient(gpu, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    _, wt, dy, _, dx_ref, _ = _case(c, s, n, h, w)
    dyd, wd = dy.to(BF16).to(gpu), wt.float().to(gpu)
    outs = []
    for _ in range(2):
        dx = torch.full(dx_ref.shape, float("nan"), dtype=BF16, device=gpu)
        N.check(N.lib().dca_ops_dwconv_dgrad(N.ptr(dyd), N.ptr(wd), N.ptr(dx), n, h, w, c, c, s, N.stream(gpu)),
                "dwconv_dgrad")
        outs.append(dx.cpu())
    assert torch.equal(outs[0], dx_ref.to(BF16)) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("c,s,n,h,w", CASES)
def test_weight_gradient(gpu, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import functional as F
    x, _, dy, _, _, dw_ref = _case(c, s, n, h, w)
    xd, dyd = x.to(BF16).to(gpu), dy.to(BF16).to(gpu)
    sink0 = torch.arange(dw_ref.numel(), dtype=torch.float32).view(dw_ref.shape) % 17 - 8
    outs = []
    for _ in range(2):
        dw = F.dwconv_wgrad(xd, dyd, s, slabs=NPARTS)
        sink = sink0.to(gpu)
        assert F.dwconv_wgrad(xd, dyd, s, out=sink, slabs=NPARTS) is sink
        outs.append((dw.cpu(), sink.cpu()))
    assert torch.equal(outs[0][0].double(), dw_ref)
    assert torch.equal(outs[0][1].double(), sink0.double() + dw_ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_mobilenet_step_and_eval(gpu):
    """A quarter-width MobileNetV1 trains one step under OpsModel: loss and every parameter gradient against the same
    module in fp32 on the CPU, with the metric and tolerance of test_resnext_step_and_eval (within 2x of stock bf16
    autocast's own error on that step, + 0.02); then an eval-mode forward against the fp32 module."""
    from distributeddataparallel_cifar10_amd.models.mobilenet import MobileNetV1
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    with torch.random.fork_rng(devices=[gpu]):  # the default generators, CPU and GPU, are left as they were found
        torch.manual_seed(0)
        ref = MobileNetV1(num_classes=10, width_mult=0.25)
        x, y = torch.randn(2, 3, 64, 64), torch.randint(0, 10, (2,))
    amp, net = copy.deepcopy(ref), copy.deepcopy(ref).to(gpu)
    model = OpsModel(net)
    assert model.kind == "mobilenet"
    loss = cross_entropy(model(x.to(gpu)), y.to(gpu))
    loss.backward()
    lref = TF.cross_entropy(ref(x), y)
    lref.backward()
    with torch.autocast("cpu", dtype=BF16):
        lamp = TF.cross_entropy(amp(x), y)
    lamp.backward()
    k, c = 2.0, 0.02
    assert abs(loss.item() - lref.item()) <= k * abs(lamp.item() - lref.item()) + c * max(1.0, lref.item())
    rows = [(n, _rel(p.grad, q.grad), _rel(r.grad, q.grad)) for (n, p), (_, q), (_, r) in
            zip(net.named_parameters(), ref.named_parameters(), amp.named_parameters())]
    bad = [(n, e, a) for n, e, a in rows if e > k * a + c]
    assert not bad, bad
    model.eval(), ref.eval(), amp.eval()
    with torch.no_grad():
        out, want = model(x.to(gpu)), ref(x)
        with torch.autocast("cpu", dtype=BF16):
            aout = amp(x)
    assert _rel(out, want) <= k * _rel(aout.float(), want) + c
