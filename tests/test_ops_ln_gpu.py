"""The LayerNorm and GELU kernels (csrc/ops_ln.hip) on the GPU against float64, ``ops.layer_norm`` and
``ops.linear(gelu=True)`` through autograd, and a VisionTransformer step under OpsModel on both of its paths."""
import pytest
import torch

from test_ops_ln import BF16, EPS, GELU_CASES, LN_CASES, gelu_case, ln_case, rel

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.mark.parametrize("m,c,offset,residual,cap,view", LN_CASES)
def test_ln_kernels_against_float64(gpu, m, c, offset, residual, cap, view):
    """hsum, y, stats, dx, dgamma, dbeta: every element written and finite, two launches bitwise equal, hsum exact; the
    relative L2 error against float64 is at most 2^-8 for the bf16 outputs (one bf16 rounding, 2^-9 per element,
    doubled) and 2^-13 for the fp32 ones (2048 x 2^-24, the worst-case bound of a fp32 sum at the widest row)."""
    from distributeddataparallel_cifar10_amd.ops import _native as N
    case = ln_case(m, c, offset, residual)

    def rows(t):  # on the device; ``view``: as the [:, 0] rows of a [M, 3, C] tensor
        if t is None or not view:
            return None if t is None else t.to(gpu)
        big = torch.randn(m, 3, c).to(BF16)
        big[:, 0] = t
        return big.to(gpu)[:, 0]

    x, res = rows(case["x"]), rows(case["res"])
    ldx = x.stride(0)
    gamma, beta, dy = case["gamma"].to(gpu), case["beta"].to(gpu), case["dy"].to(gpu)
    dres = case["dres"].to(gpu) if residual else None
    max_wg, slabs = cap or 2048, cap or 1024
    runs = []
    for _ in range(2):
        hsum, y, dx = (torch.full((m, c), NAN, dtype=BF16, device=gpu) for _ in range(3))
        stats = torch.full((m, 2), NAN, device=gpu)
        part, dgb = torch.full((slabs, 2, c), NAN, device=gpu), torch.full((2, c), NAN, device=gpu)
        N.check(N.lib().dca_ops_ln_fwd(N.ptr(x), N.ptr(res), N.ptr(gamma), N.ptr(beta), N.ptr(hsum), N.ptr(y),
                                       N.ptr(stats), m, c, ldx, EPS, max_wg, N.stream(gpu)), "ln_fwd")
        h, ldh = (hsum, c) if residual else (x, ldx)
        N.check(N.lib().dca_ops_ln_bwd(N.ptr(h), ldh, N.ptr(dy), N.ptr(dres), N.ptr(gamma), N.ptr(stats), N.ptr(dx),
                                       N.ptr(part), N.ptr(dgb), m, c, slabs, N.stream(gpu)), "ln_bwd")
        runs.append([t.cpu() for t in ((hsum,) if residual else ()) + (y, stats, dx, dgb)])
    assert all(torch.isfinite(t).all() for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    *hs, y, stats, dx, dgb = runs[0]
    assert not residual or torch.equal(hs[0], case["hsum"])
    errs = {"y": rel(y, case["y"]), "dx": rel(dx, case["dx"]), "mean": rel(stats[:, 0], case["mean"]),
            "rstd": rel(stats[:, 1], case["rstd"]), "dgamma": rel(dgb[0], case["dgamma"]),
            "dbeta": rel(dgb[1], case["dbeta"])}
    print("ln", (m, c, offset, residual, cap, view), errs)
    assert all(errs[k] <= 2 ** -8 for k in ("y", "dx")), errs
    assert all(errs[k] <= 2 ** -13 for k in ("mean", "rstd", "dgamma", "dbeta")), errs


@pytest.mark.parametrize("dy_dtype", [BF16, torch.float32])
@pytest.mark.parametrize("r,n", GELU_CASES)
def test_gelu_kernels_against_float64(gpu, r, n, dy_dtype):
    """a and dz within 2^-8, db (the column sums of the unrounded dz) within 2^-13 and bitwise repeatable; the
    accumulating form adds to a pre-filled vector."""
    from distributeddataparallel_cifar10_amd.ops import functional as F
    case = gelu_case(r, n)
    z, dy = case["z"].to(gpu), case["dy"].to(gpu).to(dy_dtype)
    a = F.gelu_fwd(z)
    (dz, db), (dz2, db2) = F.gelu_bwd(dy, z), F.gelu_bwd(dy, z)
    assert all(torch.isfinite(t).all() for t in (a, dz, db))
    assert torch.equal(db, db2) and torch.equal(dz, dz2)
    errs = rel(a, case["a"]), rel(dz, case["dz"]), rel(db, case["db"])
    print("gelu", (r, n, dy_dtype), errs)
    assert errs[0] <= 2 ** -8 and errs[1] <= 2 ** -8 and errs[2] <= 2 ** -13, errs
    sink = torch.arange(n, dtype=torch.float32, device=gpu)
    assert F.gelu_bwd(dy, z, db_into=sink)[1] is None
    assert torch.equal(sink, torch.arange(n, dtype=torch.float32, device=gpu) + db)


def test_public_functions(gpu):
    from distributeddataparallel_cifar10_amd.ops import gelu, layer_norm, linear
    from distributeddataparallel_cifar10_amd.ops import functional as F
    case = ln_case(37, 384, 0, True)
    x, res = (case[k].to(gpu).requires_grad_() for k in ("x", "res"))
    gamma, beta = (case[k].to(gpu).requires_grad_() for k in ("gamma", "beta"))
    dy, dres = case["dy"].to(gpu), case["dres"].to(gpu)
    hsum, y = layer_norm(x, gamma, beta, EPS, residual=res)
    torch.autograd.backward((hsum, y), (dres, dy))
    h0, y0, stats = F.layer_norm_fwd(x.detach(), res.detach(), gamma.detach(), beta.detach(), EPS)
    dx0, dg0, db0 = F.layer_norm_bwd(h0, dy, dres, gamma.detach(), stats)
    assert torch.equal(hsum, h0) and torch.equal(y, y0)
    assert all(torch.equal(a, b) for a, b in ((x.grad, dx0), (res.grad, dx0), (gamma.grad, dg0), (beta.grad, db0)))
    assert gamma.grad.dtype == torch.float32 and x.grad.is_contiguous()
    x.grad = None
    layer_norm(x, gamma, beta, EPS, residual=res)[1].backward(dy)  # hsum left unused: no dres
    assert torch.equal(x.grad, F.layer_norm_bwd(h0, dy, None, gamma.detach(), stats)[0])
    with torch.no_grad():
        quiet = layer_norm(x, gamma, beta, EPS)
    assert quiet.grad_fn is None and torch.equal(quiet, F.layer_norm_fwd(x.detach(), None, gamma, beta, EPS)[1])
    # linear(gelu=True) = GEMM -> gelu_fwd; its backward = gelu_bwd -> the two GEMMs of a plain linear
    g = torch.Generator().manual_seed(7)
    xin = torch.randn(37, 64, generator=g).to(BF16).to(gpu).requires_grad_()
    w, b = (t.to(gpu).requires_grad_() for t in (0.1 * torch.randn(72, 64, generator=g), torch.randn(72, generator=g)))
    da = torch.randn(37, 72, generator=g).to(BF16).to(gpu)
    out = linear(xin, w, b, out_dtype=BF16, gelu=True)
    out.backward(da)
    z = F.linear(xin.detach(), w.detach(), b.detach(), out_dtype=BF16)
    dz, db = F.gelu_bwd(da, z)
    assert torch.equal(out, F.gelu_fwd(z)) and torch.equal(b.grad, db)
    assert torch.equal(xin.grad, F.gemm(dz, F.cast_bf16(w.detach()), tb=True, out_dtype=BF16))
    zz = z.clone().requires_grad_()
    gelu(zz).backward(da)
    assert torch.equal(zz.grad, dz)
    with pytest.raises(ValueError, match="64 <= C <= 2048"):
        layer_norm(x[:, :56], gamma[:56], beta[:56])
    with pytest.raises(ValueError, match="residual has x's dtype, shape and row stride"):
        layer_norm(x, gamma, beta, residual=res[:5])
    with pytest.raises(ValueError, match="weight is a contiguous float32 tensor of shape"):
        layer_norm(x, gamma[:64], beta)
    with pytest.raises(ValueError, match="unit inner stride"):
        layer_norm(x.t(), gamma, beta)
    with pytest.raises(ValueError, match="N % 8 == 0"):
        gelu(torch.zeros(5, 12, dtype=BF16, device=gpu))


def test_vit_step_on_both_paths(gpu, monkeypatch):
    """tests/test_ops_attn_gpu.py's two-block VisionTransformer step and eval forward, with that test's bound against
    the fp32 module, on the fused LayerNorm / GELU path and on the torch path (``OPS_LN`` off)."""
    import test_ops_attn_gpu as attn_tests
    from distributeddataparallel_cifar10_amd.ops import models
    assert models.OPS_LN
    attn_tests.test_vit_step_and_eval(gpu)
    monkeypatch.setattr(models, "OPS_LN", False)
    attn_tests.test_vit_step_and_eval(gpu)
