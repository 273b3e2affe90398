"""The input-gradient dispatch of ops/functional.py::_conv_bwd, branch by branch, and the weight gradient of the same
cases, bit for bit against float64 (tests/_nn_refs.py; the references and every precondition below are proven on the CPU
by tests/test_ops_nn_refs.py).

The GEMM kernels underneath are proven by tests/test_ops_gemm_forms_gpu.py.  What is tested here is the Python that
builds the dgrad geometry (gd / gc / orow), picks the parity classes' shapes (H - ph + 1) // 2, flips the taps, chooses
between torch.empty and zeros_bf16, and threads a GradJoin through each route.

Exactness: x and dy are bf16 integers in [-3, 3], w fp32 integers in [-2, 2] (exact in bf16), a join seed / gradient sink
integers in +-8.  Every case asserts on the float64 reference that the sums of magnitudes stay below 2^24, so the fp32
accumulator holds the exact integer whatever the order or split, and dx must equal bf16(ref) and dw fp32(ref) bit for
bit.  The col2im route rounds dY . Wm to bf16 before summing taps: there |dY . Wm| <= 256 (exact in bf16; co = 8).

Route: functional.gemm and _native.check are wrapped with recording shims; each case names the branch it claims and the
records must show it -- the conv / tb / geom / orow / beta / beta_src arguments of every dgrad GEMM, whether "col2im" and
"zero" launches were checked, and the kernel the GEMM ran (printed under pytest -s).

Cases (tests/_nn_refs.py DGRAD_CASES, the smallest geometries that reach each branch): the 1x1 plain GEMM with tb=True
and with the packed W^T; the stride-1 implicit conv over weights flipped on the fly and over the packed dgrad, at the
three paddings kh - 1 - pad admits; the four parity classes (H = W and H != W) and the single-class 1x1/2 over a
zero-filled dx; the col2im fallback on odd sizes with a pack, at stride 2 without one, at C = 3 and at 5x5/2/2 (classes
of unequal padding).  C = 3 at stride 1 does not fall back: _conv_bwd's stride-1 branch asks nothing of C, so (2, 6, 6, 3,
8, 3, 1, 1) runs the implicit conv with three output columns (claimed as such, "c3_s1"), and the scalar k_col2im is
reached through functional.py by the same geometry at stride 2.

A join that holds a seed is handed in as the buffer itself (accumulate / beta = 1); a deferred masked source (dout, ReLU
bit mask; bit j of byte e / 8 = element e) goes into the 1x1 route's epilogue (beta_src / beta_mask) and through _unmask
for any other consumer.  The outputs that functional.py allocates itself cannot be pre-filled; stale memory is instead
planted in the allocator's cache (a NaN-filled block of the output's size freed just before the call), which is what
shows an element that is never written -- the odd pixels of the single-class 1x1/2 route above all."""
import pytest
import torch

import _nn_refs as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16


def _N():
    from distributeddataparallel_cifar10_amd.ops import _native
    return _native


def _F():
    from distributeddataparallel_cifar10_amd.ops import functional
    return functional


class _Recorder:
    def __init__(self, monkeypatch):
        F, N = _F(), _N()
        self.gemms, self.checks = [], []
        real_gemm, real_check = F.gemm, N.check

        def gemm(a, b, **kw):
            out = real_gemm(a, b, **kw)
            self.gemms.append(dict(kw, a=a, b=b, kernel=N.last_gemm_kernel()))
            return out

        def check(rc, what):
            self.checks.append(what)
            return real_check(rc, what)

        monkeypatch.setattr(F, "gemm", gemm)
        monkeypatch.setattr(N, "check", check)


def _setup(gpu, geom, packed):
    F = _F()
    n, h, w_, ci, co, k, s, p = geom
    d = R.dgrad_inputs(geom)
    conv = torch.nn.Conv2d(ci, co, k, stride=s, padding=p, bias=False).to(gpu)
    with torch.no_grad():
        conv.weight.copy_(d["w"].float())
    entry = None
    if packed:
        pack = F.WeightPack([conv])
        pack.pack()
        entry = pack.get(conv)
    x = d["x"].to(BF).to(gpu)
    y, st = F._conv_fwd(x, conv.weight.detach(), None, s, p, False, False, packed=entry)
    st["w_master"] = conv.weight.detach()
    assert tuple(y.shape) == tuple(d["dy"].shape)
    return d, conv, entry, st


def _plant_stale(shape, dtype, gpu):
    """Leave a NaN-filled block of this size in the allocator's cache for the next torch.empty of the same size."""
    t = torch.full(shape, float("nan"), dtype=dtype, device=gpu)
    torch.cuda.synchronize()
    del t


def _assert_route(rec, route, geom, entry, st, seeded, masked):
    n, h, w_, ci, co, k, s, p = geom
    dg = [g for g in rec.gemms if g.get("wperm") is None]
    print(f"route {route}: " + ", ".join(g["kernel"] for g in dg) + f"; checks {sorted(set(rec.checks))}")
    assert all(g["kernel"] for g in dg)
    assert ("col2im" in rec.checks) == (route == "col2im")
    assert ("zero" in rec.checks) == (route == "parity1" and not seeded)
    beta = 1.0 if seeded or masked else 0.0
    if route == "col2im":
        assert len(dg) == 1
        g = dg[0]
        assert not g.get("conv") and g.get("tb") is True and g.get("orow") is None and g.get("out") is None
        assert g.get("beta", 0.0) == 0.0 and g["b"].data_ptr() == st["wm"].data_ptr()
        return
    for g in dg:
        assert g.get("beta", 0.0) == beta, (g.get("beta"), beta)
        assert (g.get("beta_src") is not None) == (masked and route.startswith("1x1"))
        assert (g.get("beta_mask") is not None) == (masked and route.startswith("1x1"))
        assert (g.get("out") is not None) == (seeded or route.startswith("parity") or (masked and not route.startswith("1x1")))
    if route in ("1x1_tb", "1x1_packed"):
        assert len(dg) == 1 and not dg[0].get("conv") and dg[0].get("orow") is None
        assert bool(dg[0].get("tb")) == (route == "1x1_tb")
        want = st["wm"] if route == "1x1_tb" else entry["dgrad"]
        assert dg[0]["b"].data_ptr() == want.data_ptr()
    elif route in ("s1_fly", "s1_packed"):
        assert len(dg) == 1
        g = dg[0]
        gd = g["geom"]
        assert g.get("conv") == 1 and g.get("orow") is None and not g.get("tb")
        assert (gd.N, gd.H, gd.W, gd.C, gd.KH, gd.KW, gd.stride, gd.pad, gd.Ho, gd.Wo, gd.K, gd.Kp) == \
            (n, R.out_size(h, k, s, p), R.out_size(w_, k, s, p), co, k, k, 1, k - 1 - p, h, w_, k * k * co, k * k * co)
        assert g["mnk"] == (n * h * w_, ci, k * k * co)
        is_packed = entry is not None and entry["dgrad"] is not None and g["b"].data_ptr() == entry["dgrad"].data_ptr()
        assert is_packed == (route == "s1_packed")
    elif route in ("parity4", "parity1"):
        ho, wo = R.out_size(h, k, s, p), R.out_size(w_, k, s, p)
        assert len(dg) == (4 if route == "parity4" else 1)
        seen = set()
        for g in dg:
            S, ph, pw, H, W, hc, wc = g["orow"]
            gc = g["geom"]
            seen.add((ph, pw))
            assert (S, H, W, hc, wc) == (2, h, w_, (h - ph + 1) // 2, (w_ - pw + 1) // 2)
            assert g.get("conv") == 1 and (gc.N, gc.H, gc.W, gc.C, gc.stride, gc.Ho, gc.Wo) == (n, ho, wo, co, 1, hc, wc)
            assert g["mnk"] == (n * hc * wc, ci, gc.KH * gc.KW * co) and gc.K == gc.Kp == gc.KH * gc.KW * co
        assert seen == ({(0, 0), (0, 1), (1, 0), (1, 1)} if route == "parity4" else {(0, 0)})
    else:
        raise AssertionError(route)


def _cmp(what, got, ref):
    """got (device) == ref (host, the same dtype) bit for bit."""
    it = torch.int16 if ref.dtype == BF else torch.int32
    got = got.cpu().contiguous()
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (got.dtype, got.shape, ref.shape)
    bad = got.view(it) != ref.contiguous().view(it)
    print(f"ratio {what} {float(bad.any()):.4f}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at "
                                 f"{bad.nonzero()[0].tolist()}: {got[tuple(bad.nonzero()[0])]} vs "
                                 f"{ref[tuple(bad.nonzero()[0])]}")


@pytest.mark.parametrize("seeded", [False, True], ids=["fresh", "join_seed"])
@pytest.mark.parametrize("name", list(R.DGRAD_CASES))
def test_conv_dgrad_routes(gpu, monkeypatch, name, seeded):
    F = _F()
    geom, packed, route = R.DGRAD_CASES[name]
    n, h, w_, ci, co, k, s, p = geom
    d, conv, entry, st = _setup(gpu, geom, packed)
    ref = R.conv_dgrad(d["dy"], d["w"], s, p, h, w_)
    assert float((ref.abs() + 8).max()) < 2 ** 24
    dy = d["dy"].to(BF).to(gpu)
    join = None
    if seeded:
        join = F.GradJoin(2)
        assert join.contribute(d["seed"].to(BF).to(gpu)) is None
        ref = ref + d["seed"]
    else:
        _plant_stale((n, h, w_, ci), BF, gpu)
    rec = _Recorder(monkeypatch)
    dx, dw = F._conv_bwd(dy, st, True, False, x_join=join)
    torch.cuda.synchronize()
    assert dw is None
    if seeded:
        assert dx is join.buf and join.left == 0
    _cmp(f"dgrad {name} {'seeded' if seeded else 'fresh'}", dx, ref.to(BF))
    if route == "parity1" and not seeded:   # the pixels no class reaches are zero, not stale
        assert not bool(dx[:, 1::2].any()) and not bool(dx[:, :, 1::2].any())
    _assert_route(rec, route, geom, entry, st, seeded, False)


@pytest.mark.parametrize("name", list(R.DGRAD_MASKED))
def test_conv_dgrad_deferred_masked_source(gpu, monkeypatch, name):
    """dx = dY (*) W + src * bits: in the 1x1 GEMM's epilogue, or through _unmask for a 3x3 consumer."""
    F = _F()
    geom, packed, route = R.DGRAD_MASKED[name]
    n, h, w_, ci, co, k, s, p = geom
    d, conv, entry, st = _setup(gpu, geom, packed)
    ref = R.conv_dgrad(d["dy"], d["w"], s, p, h, w_) + d["seed"] * d["bits"]
    join = F.GradJoin(2, defer_ok=True)
    assert join.defer_masked(d["seed"].to(BF).to(gpu), R.pack_bits(d["bits"]).to(gpu)) is None
    _plant_stale((n, h, w_, ci), BF, gpu)
    rec = _Recorder(monkeypatch)
    dx, _ = F._conv_bwd(d["dy"].to(BF).to(gpu), st, True, False, x_join=join)
    torch.cuda.synchronize()
    _assert_route(rec, route, geom, entry, st, False, True)
    assert join.left == 0 and join.masked is None and dx is join.buf
    _cmp(f"dgrad {name}", dx, ref.to(BF))


@pytest.mark.parametrize("sunk", [False, True], ids=["fresh", "sink"])
@pytest.mark.parametrize("name", list(R.DGRAD_CASES))
def test_conv_wgrad(gpu, monkeypatch, name, sunk):
    """dw in torch's [Cout, Cin, KH, KW] layout, written fresh and accumulated into a pre-filled sink (the explicit-cols
    wperm path at C = 3 and the 1x1 cases, the implicit one elsewhere)."""
    F = _F()
    geom, packed, _ = R.DGRAD_CASES[name]
    n, h, w_, ci, co, k, s, p = geom
    d, conv, entry, st = _setup(gpu, geom, packed)
    ref = R.conv_wgrad(d["x"], d["dy"], k, s, p)
    assert float((R.conv_wgrad(d["x"].abs(), d["dy"].abs(), k, s, p) + 8).max()) < 2 ** 24
    sink = d["sink"].float().to(gpu) if sunk else None
    if not sunk:
        _plant_stale((co, ci, k, k), torch.float32, gpu)
    rec = _Recorder(monkeypatch)
    dx, dw = F._conv_bwd(d["dy"].to(BF).to(gpu), st, False, True, sink=sink)
    torch.cuda.synchronize()
    assert dx is None and (dw is None) == sunk
    (g,) = rec.gemms
    print(f"wgrad {name}: {g['kernel']}")
    assert g["wperm"] == (ci, ci, k * k) and g.get("beta", 0.0) == (1.0 if sunk else 0.0)
    assert (g.get("conv") == 2) == (st["cols"] is None)
    if name == "c3_s1" or name == "col2im_c3_s2":
        assert st["cols"] is not None and st["cols"].shape[1] == 32
    _cmp(f"wgrad {name} {'sink' if sunk else 'fresh'}", sink if sunk else dw,
         (ref + d["sink"] if sunk else ref).float())
