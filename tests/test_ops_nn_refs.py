"""The references of tests/_nn_refs.py against independent torch formulations, on the CPU, over the full case tables
of tests/test_ops_nn_forms_gpu.py and tests/test_ops_conv_dgrad_gpu.py -- the guard that a failure of those modules is the
kernel's and not the reference's -- and, on the references alone, every exactness precondition the GPU modules rely on:

  col2im          integer dcols in [-3, 3] (+ dx_old in +-8): every sum is an integer of size <= 256, exact in fp32 in any
                  order and exact in bf16.
  pool backward   integer dy: the same.  Random bf16 dy: _nn_refs.fp32_sum_exact marks the pixels whose sum is exact in
                  fp32 in any order; proven here by summing in fp32 in both tap orders.
  cross-entropy   |row[k] - max| <= 100 for every case, so the bound's rho(t) stays meaningful; labels include class 0
                  and class K - 1.
  conv gradients  integer operands: |dx| and |dw| (join seed / sink included) stay below 2^24, so an fp32 accumulator
                  holds the exact integer in any order; the col2im route's dY . Wm stays within 256 (exact in bf16).

The last test is the entry-point coverage table: every dca_ops_* function ops/_native.py declares is claimed by a named
GPU test module whose source names it (or the wrapper that calls it), or listed in EXCLUDED with the reason."""
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import _nn_refs as R

F64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("geom", R.IM2COL_GEOMS, ids=str)
def test_im2col_matches_unfold(geom):
    n, h, w, c, k, s, p = geom
    x = torch.randn(n, h, w, c, generator=R.gen(1), dtype=F64)
    cols = R.im2col(x, k, s, p)
    kk = k * k * c
    assert cols.shape[1] % 8 == 0 and 0 <= cols.shape[1] - kk < 8
    assert bool((cols[:, kk:] == 0).all())
    u = TF.unfold(_nchw(x), k, padding=p, stride=s)                    # [N, C k k, L], row c k k + tap
    u = u.view(n, c, k * k, -1).permute(0, 3, 2, 1).reshape(-1, kk)    # -> [N L, tap C + c]
    assert torch.equal(cols[:, :kk], u)
    # the GPU test's distinct integer patterns move the same way
    xi = (torch.arange(x.numel()) + 1).to(torch.int16).view(n, h, w, c)
    ci = R.im2col(xi, k, s, p)
    assert torch.equal(ci[:, :kk].to(F64), R.im2col(xi.to(F64), k, s, p)[:, :kk])


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("geom", R.COL2IM_GEOMS, ids=str)
def test_col2im_matches_fold_and_is_exact(geom, acc):
    n, h, w, c, k, s, p = geom
    g = R.gen(2)
    ho, wo = R.out_size(h, k, s, p), R.out_size(w, k, s, p)
    kk = k * k * c
    kp = (kk + 7) // 8 * 8
    d = torch.full((n * ho * wo, kp), 7.0, dtype=F64)
    d[:, :kk] = R.randint(g, -3, 3, (n * ho * wo, kk))
    old = R.randint(g, -8, 8, (n, h, w, c)) if acc else None
    dx = R.col2im(d, geom, old)
    u = d[:, :kk].view(n, ho * wo, k * k, c).permute(0, 3, 2, 1).reshape(n, c * k * k, ho * wo)
    f = TF.fold(u, (h, w), k, padding=p, stride=s).permute(0, 2, 3, 1)
    assert torch.equal(dx, f + (old if acc else 0))
    assert bool((dx == dx.round()).all()) and dx.abs().max() <= 256
    assert torch.equal(dx.to(torch.bfloat16).to(F64), dx)
    if geom == (2, 6, 6, 8, 1, 2, 0):   # three of four pixels receive nothing
        got = dx - (old if acc else 0)
        assert bool((got[:, 1::2] == 0).all()) and bool((got[:, :, 1::2] == 0).all())


_pool_x = R.pool_input


@pytest.mark.parametrize("random", [False, True])
@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_maxpool_matches_torch(case, random):
    k, s, p, h, w, c = case
    x = _pool_x(case, random).requires_grad_(True)
    y, tap = R.maxpool_fwd(x.detach(), k, s, p)
    ty, ti = TF.max_pool2d(_nchw(x), k, s, p, return_indices=True)
    assert torch.equal(y, ty.detach().permute(0, 2, 3, 1))
    ti = ti.permute(0, 2, 3, 1)
    oh = torch.arange(y.shape[1]).view(1, -1, 1, 1)
    ow = torch.arange(y.shape[2]).view(1, 1, -1, 1)
    ttap = (ti // w - (oh * s - p)) * k + (ti % w - (ow * s - p))
    assert torch.equal(tap.long(), ttap)
    dy = R.randint(R.gen(5), -3, 3, tuple(y.shape))
    (gx,) = torch.autograd.grad(ty, x, _nchw(dy))
    dx, sab, mn = R.maxpool_bwd(dy, tap, (R.POOL_N, h, w, c, k, s, p))
    assert torch.equal(dx, gx)
    assert dx.abs().max() <= 256 and bool(R.fp32_sum_exact(sab, mn).all())
    assert R.pool_family(*case) == ("k3s2" if case[:3] == (3, 2, 1) and h % 2 == 0 and w % 2 == 0 and c % 8 == 0
                                    else "generic")


def test_pool_tables_reach_both_families_and_ties():
    fams = {R.pool_family(*c) for c in R.POOL_CASES}
    assert fams == {"k3s2", "generic"} and {R.pool_family(*c) for c in R.POOL_RANDOM} == fams
    assert {c[5] for c in R.POOL_CASES} == {8, 24, 5}
    for case in R.POOL_CASES:   # most windows hold a tie for the maximum
        k, s, p, h, w, c = case
        x = _pool_x(case)
        y, _ = R.maxpool_fwd(x, k, s, p)
        cnt = torch.zeros_like(y)
        for (_, v), (_, ok) in zip(R._windows(x, k, s, p, 0.0), R._windows(torch.ones_like(x), k, s, p, 0.0)):
            cnt += ((v == y) & (ok > 0)).to(F64)
        assert float((cnt > 1).double().mean()) > 0.5, case


@pytest.mark.parametrize("case", R.POOL_RANDOM, ids=str)
def test_pool_random_dy_exactness_mask(case):
    """Where fp32_sum_exact says so, fp32 sums in either tap order equal the float64 sum; the mask covers most pixels."""
    k, s, p, h, w, c = case
    x = _pool_x(case, True)
    _, tap = R.maxpool_fwd(x, k, s, p)
    dy = torch.randn(tuple(tap.shape), generator=R.gen(9)).to(torch.bfloat16).to(F64)
    geom = (R.POOL_N, h, w, c, k, s, p)
    dx, sab, mn = R.maxpool_bwd(dy, tap, geom)
    ex = R.fp32_sum_exact(sab, mn)
    assert float(ex.double().mean()) > 0.9
    for rev in (False, True):
        d32 = R.maxpool_bwd(dy, tap, geom, dtype=torch.float32, reverse=rev)[0]
        assert torch.equal(d32.to(F64)[ex], dx[ex])


def test_maxpool_nan_rule():
    """A NaN beats any number, the first NaN wins, later numbers do not displace it."""
    x = torch.tensor([1.0, float("nan"), 5.0, float("nan")], dtype=F64).view(1, 2, 2, 1)
    y, tap = R.maxpool_fwd(x, 2, 2, 0)
    assert bool(torch.isnan(y).all()) and int(tap) == 1


@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=str)
def test_avgpool_matches_autograd(shape):
    n, hw, c = shape
    x = torch.randn(n, hw, c, generator=R.gen(3), dtype=F64, requires_grad=True)
    dy = torch.randn(n, c, generator=R.gen(4), dtype=F64)
    y = R.avgpool_fwd(x.detach())
    ty = TF.adaptive_avg_pool2d(x.permute(0, 2, 1).reshape(n, c, hw, 1), 1).view(n, c)
    assert torch.allclose(y, ty.detach(), rtol=1e-14, atol=0)
    (gx,) = torch.autograd.grad(ty, x, dy)
    assert torch.allclose(R.avgpool_bwd(dy, hw), gx, rtol=1e-14, atol=0)


@pytest.mark.parametrize("case", R.CE_CASES, ids=str)
def test_cross_entropy_matches_torch_and_preconditions(case):
    B, K, mode = case
    x, y = R.ce_inputs(B, K, mode)
    x64 = x.to(F64).requires_grad_(True)
    yc = y.clamp(0, K - 1)
    loss, mean, dl, lse, s, p = R.cross_entropy(x, y, 0.25)
    tl = TF.cross_entropy(x64, yc, reduction="none")
    assert torch.allclose(loss, tl.detach(), rtol=1e-12, atol=1e-9)     # (atol: torch cancels at the 1e4 offset)
    assert torch.allclose(mean, tl.mean().detach(), rtol=1e-12, atol=1e-9)
    (g,) = torch.autograd.grad(tl.sum() * 0.25, x64)
    assert torch.allclose(dl, g, rtol=1e-10, atol=1e-13)
    assert torch.allclose(lse, torch.logsumexp(x.to(F64), 1), rtol=1e-14, atol=0)
    # preconditions of the GPU bound
    t = x.to(F64) - x.to(F64).max(1, keepdim=True).values
    assert t.abs().max() <= R.CE_T_MAX
    if B > 1:
        assert 0 in yc.tolist() and K - 1 in yc.tolist() and (t[1].sort().values[-2] <= -40 or K == 1)
    if mode == "clamp":
        assert -1 in y.tolist() and K in y.tolist()
    if B >= 4:
        assert bool((x.max(1).values > 9000).any()) and bool((x.max(1).values < -40).any())


def test_cross_entropy_labels_cover_both_ends_at_one_row():
    modes = {(B, K): set() for B, K, _ in R.CE_CASES if B == 1}
    for B, K, m in R.CE_CASES:
        if B == 1:
            modes[(B, K)].add(int(R.ce_inputs(B, K, m)[1][0]))
    assert all(v == {0, K - 1} for (_, K), v in modes.items())


def test_e4m3_encoder_matches_torch_cast():
    codes = torch.arange(256, dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    fin = ~torch.isnan(vals)
    assert torch.equal(R.e4m3_encode(vals[fin].to(F64)), codes[fin])
    pos = vals[fin & (vals >= 0)].sort().values.to(F64)
    mid = (pos[1:] + pos[:-1]) / 2                                     # every tie, both signs
    g = R.gen(6)
    rnd = (torch.rand(20000, generator=g, dtype=F64) * 2 - 1) * 448
    tiny = (torch.rand(2000, generator=g, dtype=F64) * 2 - 1) * 2.0 ** -5
    v = torch.cat([mid, -mid, rnd, tiny, torch.tensor([0.0, -0.0, 448.0, -448.0], dtype=F64)]).float()
    assert torch.equal(R.e4m3_encode(v.to(F64)), v.to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("kind", R.FP8_KINDS)
@pytest.mark.parametrize("n", R.FP8_SIZES)
def test_quant_fp8_reference(n, kind):
    x = R.fp8_input(n, kind)
    assert torch.equal(x.to(torch.bfloat16).float(), x)               # the same values serve the bf16 and fp32 forms
    bits, q = R.quant_fp8(x)
    amax = float(x.abs().max())
    assert bits == int(torch.tensor(amax, dtype=torch.float32).view(torch.int32))
    if kind == "zero":
        assert bits == 0 and not bool(q.any())
        return
    sc = 448.0 / amax
    if kind.startswith("pow2"):                                       # exact: no assumption about the division
        assert sc == 2.0 ** round(torch.log2(torch.tensor(sc)).item())
        assert torch.equal(q, R.e4m3_encode((x.to(F64) * sc).clamp(-448, 448)))
        assert int(q.max()) >= 0xFE and (n < 1000 or int((q & 0x7F).min()) < 8)   # -448 and a subnormal are hit
    else:
        sc32 = (torch.tensor(448.0) / torch.tensor(amax)).to(F64)
        assert torch.equal(q, R.e4m3_encode((x * sc32.float()).to(F64).clamp(-448, 448)))


def test_fp8_alpha_reference():
    f = torch.float32
    for a, b, e in [(3.5, 0.75, 1.0), (0.0, 2.0, 0.5), (1.25, 0.0, 2.0), (0.0, 0.0, 3.0)]:
        want = (a / 448 if a > 0 else 1.0) * (b / 448 if b > 0 else 1.0) * e
        got = R.fp8_alpha(torch.tensor(a, dtype=f), torch.tensor(b, dtype=f), e)
        assert got.dtype == f and abs(float(got) - want) <= 4 * 2.0 ** -24 * abs(want)


@pytest.mark.parametrize("c", [1, 3, 8])
def test_nhwc8_matches_permute(c):
    x = torch.randn(2, c, 5, 7, generator=R.gen(c))
    want = TF.pad(x.permute(0, 2, 3, 1), (0, 8 - c)).to(torch.bfloat16)
    assert torch.equal(R.nchw_to_nhwc8(x), want)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw,k,p", [((10, 14), 7, 3), ((9, 11), 7, 3), ((8, 6), 3, 1), ((7, 9), 3, 1)])
def test_s2d16_matches_pixel_unshuffle_and_the_conv(c, hw, k, p):
    """The index formula against pad + pixel_unshuffle, and its purpose: the K x K / 2 conv with padding P - 1 over x is
    a ceil((K + 1) / 2)^2 stride-1 conv over y (checked through the tap identity in float64)."""
    h, w = hw
    P = p + 1
    taps = (k + 2) // 2
    ho, wo = R.out_size(h, k, 2, p), R.out_size(w, k, 2, p)
    hs, ws = ho + taps - 1, wo + taps - 1
    x = torch.randn(2, c, h, w, generator=R.gen(c + h)).to(torch.bfloat16).float()
    y = R.nchw_to_s2d16(x, hs, ws, P)
    xp = torch.zeros(2, c, 2 * hs, 2 * ws)
    hh, ww = min(h, 2 * hs - P), min(w, 2 * ws - P)
    xp[:, :, P:P + hh, P:P + ww] = x[:, :, :hh, :ww]
    u = TF.pixel_unshuffle(xp, 2).view(2, c, 4, hs, ws).permute(0, 3, 4, 2, 1).reshape(2, hs, ws, 4 * c)
    assert torch.equal(y[..., :4 * c], u.to(torch.bfloat16)) and not bool(y[..., 4 * c:].any())
    wgt = torch.randn(5, c, k, k, generator=R.gen(8), dtype=F64)
    ref = TF.conv2d(x.to(F64), wgt, stride=2, padding=p)
    w2 = torch.zeros(5, 16, taps, taps, dtype=F64)
    for i in range(taps):
        for j in range(taps):
            for ph in (0, 1):
                for pw in (0, 1):
                    kh, kw = 2 * i + ph - 1, 2 * j + pw - 1
                    if 0 <= kh < k and 0 <= kw < k:
                        w2[:, (2 * ph + pw) * c:(2 * ph + pw) * c + c, i, j] = wgt[:, :, kh, kw]
    got = TF.conv2d(y.to(F64).permute(0, 3, 1, 2), w2)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


ALL_DGRAD = {**R.DGRAD_CASES, **R.DGRAD_MASKED}


@pytest.mark.parametrize("name", list(ALL_DGRAD), ids=str)
def test_conv_gradient_references_and_exactness(name):
    geom, packed, route = ALL_DGRAD[name]
    n, h, w_, ci, co, k, s, p = geom
    d = R.dgrad_inputs(geom)
    x = d["x"].clone().requires_grad_(True)
    wt = d["w"].clone().requires_grad_(True)
    y = TF.conv2d(_nchw(x), wt, stride=s, padding=p)
    assert tuple(y.shape[2:]) == tuple(d["dy"].shape[1:3])
    gx, gw = torch.autograd.grad(y, (x, wt), _nchw(d["dy"]))
    dx, dw = R.conv_dgrad(d["dy"], d["w"], s, p, h, w_), R.conv_wgrad(d["x"], d["dy"], k, s, p)
    assert torch.equal(dx, gx) and torch.equal(dw, gw)                 # integers: float64 is exact either way
    # the col2im formulation: dY . Wm scattered by col2im
    dcols = d["dy"].reshape(-1, co) @ R.weight_matrix(d["w"])
    assert torch.equal(R.col2im(dcols, (n, h, w_, ci, k, s, p)), dx)
    if s == 2:
        assert torch.equal(R.parity_dgrad(d["dy"], d["w"], p, h, w_), dx)
    # exactness preconditions
    for t in (d["x"], d["dy"]):
        assert t.abs().max() <= 3 and torch.equal(t.to(torch.bfloat16).to(F64), t)
    assert d["w"].abs().max() <= 2 and d["seed"].abs().max() <= 8 and d["sink"].abs().max() <= 8
    assert (dx.abs() + d["seed"].abs()).max() < 2 ** 24 and (dw.abs() + d["sink"].abs()).max() < 2 ** 24
    # every partial sum is bounded by the sum of magnitudes
    absx = R.conv_dgrad(d["dy"].abs(), d["w"].abs(), s, p, h, w_) + 8
    absw = R.conv_wgrad(d["x"].abs(), d["dy"].abs(), k, s, p) + 8
    assert absx.max() < 2 ** 24 and absw.max() < 2 ** 24
    if route == "col2im":
        assert co == 8 and dcols.abs().max() <= 256
    if route.startswith("parity"):
        assert h % 2 == 0 and w_ % 2 == 0 and s == 2
    if route == "s1_fly" or route == "s1_packed":
        assert s == 1 and 0 <= k - 1 - p <= k - 1


def test_parity_classes_of_the_table():
    """3x3/2/1: four classes of 1x1, 1x2, 2x1 and 2x2 taps, all with padding 0; 1x1/2/0: the one class (0, 0) = W^T;
    5x5/2/2: classes with unequal padding (WeightPack._parity_classes returns None: the col2im route)."""
    w3 = torch.randn(16, 8, 3, 3, generator=R.gen(1))
    c3 = R.parity_classes(w3, 1)
    assert {k: (len(v[0]), len(v[1]), v[2]) for k, v in c3.items()} == {
        (0, 0): (1, 1, (0, 0)), (0, 1): (1, 2, (0, 0)), (1, 0): (2, 1, (0, 0)), (1, 1): (2, 2, (0, 0))}
    assert c3[(1, 1)][0] == [2, 0]
    w1 = torch.randn(16, 8, 1, 1, generator=R.gen(2))
    c1 = R.parity_classes(w1, 0)
    assert list(c1) == [(0, 0)] and torch.equal(c1[(0, 0)][3], w1[:, :, 0, 0].to(F64).t())
    c5 = R.parity_classes(torch.randn(8, 8, 5, 5, generator=R.gen(3)), 2)
    assert c5[(0, 1)][2] == (1, 0)
    for wt, p in ((w3, 1), (w1, 0)):
        dy = torch.randn(2, 3, 4, 16, generator=R.gen(4), dtype=F64)
        assert torch.allclose(R.parity_dgrad(dy, wt, p, 6, 8), R.conv_dgrad(dy, wt, 2, p, 6, 8), rtol=1e-12, atol=1e-12)


def test_pack_bits_order():
    bits = torch.zeros(16)
    bits[3] = bits[8] = 1
    assert R.pack_bits(bits).tolist() == [8, 1]


# ---------------------------------------------------------------------------------------------------------------------
# entry-point coverage
# ---------------------------------------------------------------------------------------------------------------------
NN, DG = "test_ops_nn_forms_gpu.py", "test_ops_conv_dgrad_gpu.py"
BN, GF, OPS = "test_ops_bn_gpu.py", "test_ops_gemm_forms_gpu.py", "test_ops_gpu.py"
# entry point -> (GPU test module, the token in its source that names the entry point or the wrapper that calls it)
CLAIMED = {
    "dca_ops_gemm": (GF, "dca_ops_gemm"), "dca_ops_gemm_last_route": (GF, "dca_ops_gemm_last_route"),
    "dca_ops_bn_plan": (BN, "bn_plan("), "dca_ops_bn_fwd": (BN, "dca_ops_bn_fwd("),
    "dca_ops_bn_fwd_parts": (BN, "dca_ops_bn_fwd_parts"), "dca_ops_bn_eval": (BN, "dca_ops_bn_eval"),
    "dca_ops_bn_bwd": (BN, "dca_ops_bn_bwd"),
    "dca_ops_bn_pool_fwd_parts": (OPS, "pool=True"), "dca_ops_bn_pool_bwd": (OPS, "pool=True"),
    "dca_ops_dy_prep": (OPS, "dy_prep("), "dca_ops_sgd": (OPS, "sgd_step_("),
    "dca_ops_pack_weights": (OPS, "WeightPack("),
    "dca_ops_adam": ("test_adam_gpu.py", "adam_step_("), "dca_ops_clip_coef": ("test_clip_gpu.py", "clip_coef_("),
    "dca_ops_clip_state_words": ("test_clip_gpu.py", "clip_state("),
    "dca_ops_im2col": (NN, "dca_ops_im2col"), "dca_ops_col2im": (NN, "dca_ops_col2im"),
    "dca_ops_maxpool_fwd": (NN, "dca_ops_maxpool_fwd"), "dca_ops_maxpool_bwd": (NN, "dca_ops_maxpool_bwd"),
    "dca_ops_avgpool_fwd": (NN, "dca_ops_avgpool_fwd"), "dca_ops_avgpool_bwd": (NN, "dca_ops_avgpool_bwd"),
    "dca_ops_cross_entropy": (NN, "dca_ops_cross_entropy"), "dca_ops_zero": (NN, "zeros_bf16("),
    "dca_ops_scale_dev": (NN, "test_scale_dev"), "dca_ops_cast_bf16": (NN, "cast_bf16("),
    "dca_ops_add_i64": (NN, "add_one_i64("), "dca_ops_gather_cols": (NN, "gather_cols("),
    "dca_ops_quant_fp8": (NN, "quantize_fp8("), "dca_ops_fp8_alpha": (NN, "fp8_alpha("),
    "dca_ops_pack_gather": (NN, "WeightPack("), "dca_ops_nchw_to_nhwc8": (NN, "nchw_to_nhwc8("),
    "dca_ops_nchw_to_s2d16": (NN, "dca_ops_nchw_to_s2d16"),
}
# an entry point, or "entry point: path" for a path of a claimed one that stays out
EXCLUDED = {
    "dca_ops_last_error": "Returns the message of a failed call; it runs only when a launcher rejects its arguments.",
    "dca_ops_abi_version": "Checked against ABI_VERSION by _native.lib() on every load.",
    "dca_ops_pack_desc_size": "Checked against the ctypes mirror by _native.lib() on every load.",
    "dca_ops_gather_desc_size": "Checked against the ctypes mirror by _native.lib() on every load.",
    "dca_ops_gemm_route": "A pure host function, tested without a device in tests/test_native_build.py.",
    "dca_ops_maxpool_fwd: k_maxpool_*<long>": "The 64-bit index instantiations need more than 2^31 elements.",
    "dca_ops_maxpool_bwd: k_maxpool_*<long>": "The 64-bit index instantiations need more than 2^31 elements.",
    "dca_ops_avgpool_bwd: fall-through past 2^31": "The scalar kernel at C % 8 == 0 needs more than 2^31 elements.",
}


def test_every_entry_point_is_claimed_or_excluded():
    src = open(os.path.join(HERE, "..", "distributeddataparallel_cifar10_amd", "ops", "_native.py")).read()
    body = src[src.index("def _declare(lib):"):src.index("def library_path")]
    declared = set(re.findall(r"lib\.(dca_ops_\w+)\.", body))
    assert len(declared) > 30
    whole = {k for k in EXCLUDED if ":" not in k}
    partial = {k.split(":")[0] for k in EXCLUDED if ":" in k}
    assert all(len(r.split()) > 3 and r.endswith(".") for r in EXCLUDED.values())
    assert not (set(CLAIMED) & whole), set(CLAIMED) & whole
    assert set(CLAIMED) | whole == declared, (declared - set(CLAIMED) - whole, (set(CLAIMED) | whole) - declared)
    assert partial <= set(CLAIMED)
    for name, (module, token) in CLAIMED.items():
        text = open(os.path.join(HERE, module)).read()
        assert "pytest.mark.gpu" in text, module
        assert token in text, (name, module, token)
