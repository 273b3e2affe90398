"""The grouped 3x3 kernels (csrc/ops_gconv.hip) on an MI355X against torch's float64 grouped conv (tests/test_ops_gconv.py):
integer inputs make every fp32 sum exact, so forward, input gradient and weight gradient are compared bit for bit."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as TF

from test_ops_gconv import gconv_inputs, gconv_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# ragged 16-pixel tiles, odd sizes under stride 2, block counts that are no power of two, two images; one real width
CASES = [(cg, c, s, n, h, w) for cg, c in ((4, 48), (8, 32), (16, 48), (32, 96)) for s in (1, 2)
         for n, h, w in ((2, 5, 19), (1, 7, 17))] + [(4, 128, 1, 1, 4, 56)]
NPARTS = 4  # statistics rows / weight-gradient slabs: fewer than the units of some cases, more than those of others


@functools.lru_cache(maxsize=None)
def _case(cg, c, s, n, h, w):  # inputs and float64 reference, computed once per case and never modified
    x, wt, dy = gconv_inputs(cg, c, s, n, h, w)
    return (x, wt, dy) + gconv_ref(x, wt, dy, s, c // cg)


def _packed(wt, groups, gpu):
    from distributeddataparallel_cifar10_amd.ops import functional as F
    wd = wt.float().to(gpu)
    return F.gconv_pack(wd, F.gconv_entry(wd, groups))


@pytest.mark.parametrize("cg,c,s,n,h,w", CASES)
def test_forward_and_bn_partial_sums(gpu, cg, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    x, wt, _, y_ref, _, _ = _case(cg, c, s, n, h, w)
    e = _packed(wt, c // cg, gpu)
    xd = x.to(BF16).to(gpu)
    shift = (0.25 * (torch.arange(c) % 4 + 1) * (1 - 2 * (torch.arange(c) % 2))).float()  # dyadic, non-zero
    outs = []
    for _ in range(2):
        y = torch.full(y_ref.shape, float("nan"), dtype=BF16, device=gpu)
        part = torch.full((NPARTS, c, 2), float("nan"), device=gpu)
        N.check(N.lib().dca_ops_gconv_fwd(N.ptr(xd), N.ptr(e["fwd"]), N.ptr(y), N.ptr(part), N.ptr(shift.to(gpu)),
                                          NPARTS, n, h, w, c, c // cg, s, N.stream(gpu)), "gconv_fwd")
        outs.append((y.cpu(), part.cpu()))
    want = y_ref.to(BF16)
    assert torch.equal(outs[0][0], want)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    v = want.double().view(-1, c) - shift.double()
    got = outs[0][1].double().sum(0)  # [c, 2]
    tol = NPARTS * 2.0 ** -24  # one fp32 rounding per row summed
    assert ((got[:, 0] - v.sum(0)).abs() <= tol * v.abs().sum(0)).all()
    assert ((got[:, 1] - (v * v).sum(0)).abs() <= tol * (v * v).sum(0)).all()


@pytest.mark.parametrize("cg,c,s,n,h,w", CASES)
def test_input_gradient(gpu, cg, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    _, wt, dy, _, dx_ref, _ = _case(cg, c, s, n, h, w)
    e = _packed(wt, c // cg, gpu)
    dyd = dy.to(BF16).to(gpu)
    outs = []
    for _ in range(2):
        dx = torch.full(dx_ref.shape, float("nan"), dtype=BF16, device=gpu)
        N.check(N.lib().dca_ops_gconv_dgrad(N.ptr(dyd), N.ptr(e["dgrad"]), N.ptr(dx), n, h, w, c, c // cg, s,
                                            N.stream(gpu)), "gconv_dgrad")
        outs.append(dx.cpu())
    assert torch.equal(outs[0], dx_ref.to(BF16)) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("cg,c,s,n,h,w", CASES)
def test_weight_gradient(gpu, cg, c, s, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import functional as F
    x, _, dy, _, _, dw_ref = _case(cg, c, s, n, h, w)
    xd, dyd = x.to(BF16).to(gpu), dy.to(BF16).to(gpu)
    sink0 = torch.arange(dw_ref.numel(), dtype=torch.float32).view(dw_ref.shape) % 17 - 8
    outs = []
    for _ in range(2):
        dw = F.gconv_wgrad(xd, dyd, c // cg, s, slabs=NPARTS)
        sink = sink0.to(gpu)
        assert F.gconv_wgrad(xd, dyd, c // cg, s, out=sink, slabs=NPARTS) is sink
        outs.append((dw.cpu(), sink.cpu()))
    assert torch.equal(outs[0][0].double(), dw_ref)
    assert torch.equal(outs[0][1].double(), sink0.double() + dw_ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_resnext_step_and_eval(gpu):
    """A ResNeXt with grouped convs of Cg 4 / 8 / 16 / 32 trains one step under OpsModel: loss and every parameter
    gradient against the same module in fp32 on the CPU, with the metric and tolerance of test_ops_resnet_step
    (tests/test_ops_gpu.py:369-379: within 2x of stock bf16 autocast's own error on that step, + 0.02); then an
    eval-mode forward against the fp32 module."""
    from distributeddataparallel_cifar10_amd.models.resnet50 import ResNet
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    with torch.random.fork_rng(devices=[gpu]):  # the default generators, CPU and GPU, are left as they were found
        torch.manual_seed(0)
        ref = ResNet([1, 1, 1, 1], num_classes=10, zero_init_residual=False, groups=8, width_per_group=4)
        x, y = torch.randn(2, 3, 64, 64), torch.randint(0, 10, (2,))
    amp, net = copy.deepcopy(ref), copy.deepcopy(ref).to(gpu)
    model = OpsModel(net)
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
