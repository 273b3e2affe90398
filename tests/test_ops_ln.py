"""Fused residual-add LayerNorm and GELU on the ops path (csrc/ops_ln.hip), the parts that need no GPU: the launchers'
shape rules, the argument checks of ``ops.layer_norm`` / ``ops.gelu`` / ``ops.linear(gelu=True)``, and the float64
references that tests/test_ops_ln_gpu.py uses."""
import functools
import math

import pytest
import torch

BF16 = torch.bfloat16
EPS = 1e-5
# (M, C, offset, residual, workgroup cap, rows as [:, 0] views).  200: a ragged chunk count; 1000 rows under a cap of 5
# workgroups of 32 lane groups: each group walks 6 or 7 rows and the slab sum takes 5 slabs
LN_CASES = [(1, 64, 0, False, 0, False), (3, 192, 0, True, 0, False), (5, 200, 8, True, 0, False),
            (37, 384, 0, True, 0, False), (67, 768, 8, False, 0, False), (9, 1024, 0, True, 0, False),
            (4, 2048, 8, True, 0, False), (1000, 192, 0, True, 5, False), (2, 192, 0, True, 0, True)]
GELU_CASES = [(1, 8), (5, 72), (67, 768), (130, 200)]  # (R, N)


def rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def ln_case(m, c, offset, residual):
    """Seeded bf16 x (``offset`` 8: 8 + 0.25 randn, which defeats a one-pass variance), residual, dy and dres, fp32
    gamma and beta; and the float64 composition on those values, with x + residual rounded to bf16 before the
    normalisation: hsum, y, mean, rstd, dx (with dres joined), dgamma, dbeta."""
    g = torch.Generator().manual_seed(10000 * c + 10 * m + int(residual))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    case = {"x": (offset + 0.25 * rn(m, c) if offset else rn(m, c)).to(BF16), "dy": rn(m, c).to(BF16),
            "gamma": 1 + 0.5 * rn(c), "beta": rn(c), "res": None, "dres": None}
    h = case["x"].double()
    if residual:
        case["res"], case["dres"] = rn(m, c).to(BF16), rn(m, c).to(BF16)
        h = (h + case["res"].double()).to(BF16).double()
    h.requires_grad_()
    gamma, beta = case["gamma"].double().requires_grad_(), case["beta"].double().requires_grad_()
    mean = h.mean(-1, keepdim=True)
    rstd = ((h - mean).square().mean(-1, keepdim=True) + EPS).rsqrt()
    y = (h - mean) * rstd * gamma + beta
    y.backward(case["dy"].double())
    dx = h.grad + (case["dres"].double() if residual else 0)
    case.update(hsum=h.detach().to(BF16), y=y.detach(), mean=mean.detach()[:, 0], rstd=rstd.detach()[:, 0], dx=dx,
                dgamma=gamma.grad, dbeta=beta.grad)
    return case


@functools.lru_cache(maxsize=None)
def gelu_case(r, n):
    """Seeded bf16 z = 2.5 randn and dy; float64 a = gelu(z) (erf form), dz = dy gelu'(z) and its column sums db."""
    g = torch.Generator().manual_seed(1000 * n + r)
    z, dy = (2.5 * torch.randn(r, n, generator=g)).to(BF16), torch.randn(r, n, generator=g).to(BF16)
    zd = z.double()
    cdf = 0.5 * (1 + torch.erf(zd / math.sqrt(2)))
    dz = dy.double() * (cdf + zd * torch.exp(-0.5 * zd * zd) / math.sqrt(2 * math.pi))
    return {"z": z, "dy": dy, "a": zd * cdf, "dz": dz, "db": dz.sum(0)}


@pytest.mark.parametrize("m,c,ldx,ok", [(1, 64, 64, True), (3, 192, 192, True), (5, 200, 200, True),
                                        (4, 2048, 2048, True), (2, 192, 576, True),
                                        (1, 56, 56, False), (1, 2056, 2056, False), (1, 196, 196, False),
                                        (2, 192, 184, False), (2, 192, 196, False), (0, 192, 192, False),
                                        (1 << 20, 2048, 2048, False),    # 2^31 elements
                                        ((1 << 20) - 1, 2048, 2048, True)])
def test_ln_rule_boundaries(m, c, ldx, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    assert (N.lib().dca_ops_ln_rule(m, c, ldx) == 0) == ok
    if not ok:
        assert b"LayerNorm rule is" in N.lib().dca_ops_last_error()


@pytest.mark.parametrize("r,n,ok", [(1, 8, True), (130, 200, True), (5, 12, False), (0, 8, False),
                                    (1 << 28, 8, False)])
def test_gelu_rule_boundaries(r, n, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    assert (N.lib().dca_ops_gelu_rule(r, n) == 0) == ok
    if not ok:
        assert b"GELU rule is" in N.lib().dca_ops_last_error() and b"N % 8 == 0" in N.lib().dca_ops_last_error()


def test_argument_checks():
    from distributeddataparallel_cifar10_amd.ops import gelu, layer_norm, linear
    w, b = torch.ones(64), torch.zeros(64)
    with pytest.raises(TypeError, match="x is a bfloat16 tensor"):
        layer_norm(torch.zeros(2, 64), w, b)
    with pytest.raises(TypeError, match="residual is a bfloat16 tensor"):
        layer_norm(torch.zeros(2, 64, dtype=BF16), w, b, residual=torch.zeros(2, 64))
    with pytest.raises(ValueError, match="GPU tensors"):
        layer_norm(torch.zeros(2, 64, dtype=BF16), w, b)
    with pytest.raises(TypeError, match="bfloat16"):
        gelu(torch.zeros(2, 8))
    with pytest.raises(ValueError, match="GPU tensors"):
        gelu(torch.zeros(2, 8, dtype=BF16))
    x, lw = torch.zeros(2, 16, dtype=BF16), torch.zeros(8, 16)
    with pytest.raises(ValueError, match="gelu=True is not available together with relu=True or fp8=True"):
        linear(x, lw, relu=True, gelu=True, out_dtype=BF16)
    with pytest.raises(ValueError, match="gelu=True is not available together with relu=True or fp8=True"):
        linear(x, lw, fp8=True, gelu=True, out_dtype=BF16)
    with pytest.raises(ValueError, match="gelu=True returns bfloat16"):
        linear(x, lw, gelu=True)


def test_references_are_what_torch_computes():
    """The float64 references against torch's own float64 layer_norm and gelu (and their autograd)."""
    case = ln_case(5, 200, 8, True)
    h = case["hsum"].double().requires_grad_()
    y = torch.nn.functional.layer_norm(h, (200,), case["gamma"].double(), case["beta"].double(), EPS)
    y.backward(case["dy"].double())
    assert rel(case["y"], y) < 1e-12 and rel(case["dx"], h.grad + case["dres"].double()) < 1e-12
    assert torch.equal(case["hsum"], (case["x"].float() + case["res"].float()).to(BF16))
    gc = gelu_case(5, 72)
    z = gc["z"].double().requires_grad_()
    a = torch.nn.functional.gelu(z)
    a.backward(gc["dy"].double())
    assert rel(gc["a"], a) < 1e-12 and rel(gc["dz"], z.grad) < 1e-12
