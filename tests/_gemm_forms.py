"""The case table of the GEMM epilogue tests: every kernel instantiation of csrc/ops_gemm_route.hip GEMM_KERNELS at the
smallest shape the route sends to it, crossed with the epilogue forms its family's route admits.

Read by tests/test_native_build.py::test_gemm_form_cases_cover_the_table (no device: every case and form must route to
the kernel it claims, and claimed + EXCLUDED must be the whole table) and by tests/test_ops_gemm_forms_gpu.py (the same
GemmArgs with real pointers, against float64).  ``gemm_fields`` is the one place a case and a form become GemmArgs
fields, so both tiers see the same shape fields and the same null / non-null pointers.  No GPU import here."""
from dataclasses import dataclass, field
from typing import Optional, Tuple


@dataclass(frozen=True)
class Form:
    """One set of epilogue options.  route: claims this form adds to (or overrides in) its case's."""
    name: str
    out: str = "bf16"                  # "bf16" | "f32"
    alpha: float = 1.0
    alpha_dev: Optional[float] = None  # value of the device-side factor
    bias: bool = False
    beta: float = 0.0
    relu: bool = False
    ldc_pad: int = 0                   # ldc = N + ldc_pad
    stats: bool = False                # col_stats + stats_shift (ternary operands)
    orow: bool = False                 # S = 2 row remap into the (ph, pw) = (1, 0) parity class
    mask: bool = False                 # beta_src + beta_mask
    wperm: Optional[Tuple[int, int, int]] = None   # (C, Cpad, T)
    amax: bool = False                 # fp8 amax_a / amax_b
    route: dict = field(default_factory=dict)


_ALL = dict(alpha=0.25, alpha_dev=2.0, bias=True, beta=-2.0, relu=True)
# gemm_epilogue (k_gemm, k_gemm_glds)
TILE = (Form("f32", out="f32"), Form("bf16"), Form("alpha", alpha=0.5),
        Form("alpha_dev_f32", out="f32", alpha=0.25, alpha_dev=2.0), Form("bias", bias=True),
        Form("beta_f32", out="f32", beta=-2.0), Form("beta_bf16", beta=1.0), Form("relu", relu=True),
        Form("all", **_ALL), Form("all_f32", out="f32", **_ALL),
        Form("ldc", beta=1.0, ldc_pad=8), Form("ldc_f32", out="f32", bias=True, ldc_pad=8),
        Form("stats", bias=True, stats=True), Form("stats_f32", out="f32", alpha=0.5, stats=True),
        Form("orow", orow=True), Form("orow_beta", orow=True, bias=True, beta=1.0))
# the partial (N = 204, ldc = 208) and the scalar (N = 203, ldc = 203) column group
TILE_COLS = (Form("f32", out="f32"), Form("bf16"), Form("beta_bf16", beta=1.0), Form("all", **_ALL),
             Form("all_f32", out="f32", **_ALL), Form("stats", bias=True, stats=True))
# the same options through the fp32 slab and k_gemm_splitk_reduce
SPLIT = (Form("f32", out="f32"), Form("bf16"), Form("all", **_ALL), Form("all_f32", out="f32", **_ALL),
         Form("ldc", beta=1.0, ldc_pad=8), Form("ldc_f32", out="f32", bias=True, ldc_pad=8))
# store_quarters_256 (k_gemm_pp, k_gemm_pp4)
PP = (Form("f32", out="f32"), Form("bf16"), Form("alpha_bias_relu", alpha=0.5, bias=True, relu=True),
      Form("beta_bf16", beta=1.0), Form("ldc", bias=True, ldc_pad=8), Form("stats", stats=True))
MASKED = (Form("masked", beta=1.0, mask=True), Form("masked_all", alpha=0.5, bias=True, beta=-2.0, mask=True))
# k_gemm_stream's own epilogue
STREAM = (Form("bf16"), Form("alpha_bias", alpha=0.25, alpha_dev=2.0, bias=True), Form("stats", bias=True, stats=True),
          Form("ldc", alpha=0.5, stats=True, ldc_pad=8))
STREAM_BETA = (Form("beta", beta=1.0), Form("beta_all", alpha=0.5, bias=True, beta=-2.0, ldc_pad=8),
               Form("beta_stats", beta=1.0, stats=True))
# row-ring and direct convolutions (bf16 output, no beta / ReLU)
ROWS = (Form("bf16"), Form("alpha", alpha=0.5), Form("bias_stats", bias=True, stats=True),
        Form("all_ldc", alpha=0.25, alpha_dev=2.0, bias=True, stats=True, ldc_pad=8))
# weight-gradient kernels: always the slab and k_gemm_splitk_reduce
WGRAD = (Form("f32", out="f32"), Form("acc", out="f32", alpha=0.5, beta=1.0), Form("bf16"),
         Form("bf16_acc", alpha=0.5, bias=True, beta=-2.0))
WPERM = (Form("wperm", out="f32", wperm=(3, 8, 9)), Form("wperm_acc", out="f32", alpha=0.5, beta=1.0, wperm=(3, 8, 9)))
FP8 = (Form("f32", out="f32"), Form("bf16"), Form("bias_relu", bias=True, relu=True),
       Form("amax_f32", out="f32", amax=True), Form("amax_all", amax=True, alpha=0.5, bias=True, beta=-2.0))


@dataclass(frozen=True)
class Case:
    """One routed shape.  plain (conv 0): mnk; conv 1 / 2: geom = (n, h, w, c, co, kh, kw, stride, pad), conv 2 being
    the weight gradient of that convolution.  lda / ldb None: the operand's natural width.  ws: a workspace is passed
    (always with splits > 1 or a wperm form).  route: the claimed splits / reduce / masked_copy."""
    id: str
    kernel: str
    forms: Tuple[Form, ...]
    conv: int = 0
    mnk: Optional[Tuple[int, int, int]] = None
    geom: Optional[Tuple[int, ...]] = None
    ta: int = 0
    tb: int = 0
    fp8: int = 0
    lda: Optional[int] = None
    ldb: Optional[int] = None
    splits: int = 1
    ws: bool = False
    stream: bool = False               # the masked source is applied in the kernel's own epilogue
    route: dict = field(default_factory=dict)

    @property
    def out_hw(self):
        n, h, w, c, co, kh, kw, s, p = self.geom
        return (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1

    @property
    def shape(self):
        if not self.conv:
            return self.mnk
        n, h, w, c, co, kh, kw, s, p = self.geom
        ho, wo = self.out_hw
        return (n * ho * wo, co, kh * kw * c) if self.conv == 1 else (co, kh * kw * c, n * ho * wo)


def orow_grid(M):
    """(n, Ho, Wo, H, W, ph, pw) of the S = 2 remap a case of M rows uses: M = n Ho Wo, out rows n H W."""
    wo = max(d for d in range(1, 18) if M % d == 0)
    ho = max(d for d in range(1, 9) if (M // wo) % d == 0)
    return M // (wo * ho), ho, wo, 2 * ho, 2 * wo, 1, 0


def claims(case, form):
    """name / splits / reduce / masked_copy this (case, form) claims of the route."""
    c = dict(name=case.kernel, masked_copy=int(form.mask and not case.stream),
             reduce=int(case.ws or case.splits > 1 or form.wperm is not None))
    c.update(case.route)
    c.update(form.route)
    return c


def gemm_fields(case, form):
    """GemmArgs fields of (case, form); a pointer field is None (null) or 0 (the caller's buffer goes there)."""
    M, N, K = case.shape
    f = dict(A=0, B=0, C=0, M=M, N=N, K=K, alpha=form.alpha, beta=form.beta, ta=case.ta, tb=case.tb, fp8=case.fp8,
             relu=int(form.relu), out_bf16=int(form.out == "bf16"), splits=case.splits, k_per_split=0, conv=case.conv,
             ldc=N + form.ldc_pad)
    f["lda"] = 0 if case.conv == 1 else case.lda if case.lda is not None else (M if case.ta else K)
    f["ldb"] = 0 if case.conv == 2 else case.ldb if case.ldb is not None else (N if case.tb else K)
    if case.conv:
        n, h, w, c, co, kh, kw, s, p = case.geom
        ho, wo = case.out_hw
        f.update(cN=n, cH=h, cW=w, cC=c, cKH=kh, cKW=kw, cS=s, cP=p, cHo=ho, cWo=wo)
    if case.ws or case.splits > 1 or form.wperm is not None:
        f["ws"] = 0
    if form.bias:
        f["bias"] = 0
    if form.alpha_dev is not None:
        f["alpha_dev"] = 0
    if form.stats:
        f["col_stats"] = f["stats_shift"] = 0
    if form.amax:
        f["amax_a"] = f["amax_b"] = 0
    if form.mask:
        f["beta_src"] = f["beta_mask"] = 0
    if form.wperm is not None:
        f["wperm_C"], f["wperm_Cpad"], f["wperm_T"] = form.wperm
    if form.orow:
        n, ho, wo, H, W, ph, pw = orow_grid(M)
        f.update(orow_S=2, orow_ph=ph, orow_pw=pw, orow_H=H, orow_W=W, orow_Ho=ho, orow_Wo=wo)
    return f


def _rows3x3(w, c=64):
    return (2, 5, w, c, c, 3, 3, 1, 1)


def _s2d(w):
    return (1, 8, w, 16, 64, 4, 4, 1, 0)


_WG = dict(ta=1, tb=1, ws=True)
_WGC = dict(conv=2, ta=1, ws=True, splits=4, forms=WGRAD)
CASES = (
    # ---- k_gemm: register-staged (a transposed operand, or rows that are not 16-B aligned) ----
    Case("gemm128_tt_single", "k_gemm<false, 128>", TILE, mnk=(136, 200, 100), ta=1, tb=1),
    Case("gemm128_tt_double", "k_gemm<false, 128>", TILE, mnk=(136, 200, 520), ta=1, tb=1),
    Case("gemm128_dgrad_tb", "k_gemm<false, 128>", TILE, mnk=(200, 136, 72), tb=1),
    Case("gemm128_nt_lda100", "k_gemm<false, 128>", TILE, mnk=(136, 200, 100)),
    Case("gemm128_n204_ldc208", "k_gemm<false, 128>", tuple(Form(**dict(f.__dict__, ldc_pad=4)) for f in TILE_COLS),
         mnk=(136, 204, 100), ta=1, tb=1, lda=136, ldb=208),
    Case("gemm128_n203_ldc203", "k_gemm<false, 128>", TILE_COLS, mnk=(136, 203, 100), ta=1, tb=1, lda=136, ldb=208),
    Case("gemm64_ta", "k_gemm<false, 64>", TILE, mnk=(200, 40, 100), ta=1),
    Case("gemm64_77x10x37", "k_gemm<false, 64>", TILE, mnk=(77, 10, 37)),
    # ---- k_gemm_glds: LDS-DMA staging ----
    Case("glds128_w4", "k_gemm_glds<false, 128, 4>", TILE, mnk=(200, 136, 128)),
    Case("glds128_w8", "k_gemm_glds<false, 128, 8>", TILE, mnk=(200, 136, 640)),
    Case("glds128_n204_ldc208", "k_gemm_glds<false, 128, 4>",
         tuple(Form(**dict(f.__dict__, ldc_pad=4)) for f in TILE_COLS), mnk=(200, 204, 128)),
    Case("glds128_n203_ldc203", "k_gemm_glds<false, 128, 4>", TILE_COLS, mnk=(200, 203, 128)),
    Case("glds128_split3", "k_gemm_glds<false, 128, 4>", SPLIT, mnk=(200, 136, 640), splits=3,
         route=dict(splits=3, k_per_split=256)),
    Case("glds64_w4", "k_gemm_glds<false, 64, 4>", TILE, mnk=(200, 64, 128)),
    Case("glds64_w8", "k_gemm_glds<false, 64, 8>", TILE, mnk=(200, 48, 640)),
    Case("glds128_beta_k192", "k_gemm_glds<false, 128, 4>", (Form("beta", beta=1.0),), mnk=(16424, 128, 192)),
    Case("gemm128_tb_split2", "k_gemm<false, 128>", SPLIT, mnk=(136, 200, 130), tb=1, splits=2,
         route=dict(splits=2, k_per_split=128)),
    # ---- fp8 ----
    Case("glds128_f8_w4", "k_gemm_glds<true, 128, 4>", FP8, mnk=(160, 144, 256), fp8=1),
    Case("glds128_f8_w8", "k_gemm_glds<true, 128, 8>", FP8, mnk=(160, 144, 1280), fp8=1),
    Case("glds64_f8_w4", "k_gemm_glds<true, 64, 4>", FP8, mnk=(160, 48, 256), fp8=1),
    Case("glds64_f8_w8", "k_gemm_glds<true, 64, 8>", FP8, mnk=(160, 48, 1280), fp8=1),
    # ---- ping-pong 256 x 256 tiles: 160 tiles with an M tail ----
    Case("pp256", "k_gemm_pp<256>", PP, mnk=(2500, 4096, 520)),
    Case("pp4", "k_gemm_pp4<false>", PP, mnk=(2500, 4096, 512)),
    Case("pp4_masked", "k_gemm_pp4<false>", MASKED, mnk=(2560, 4096, 512)),
    Case("pp4_conv", "k_gemm_pp4<true>", PP, conv=1, geom=(16, 51, 51, 64, 256, 3, 3, 1, 1)),
    # ---- persistent stream kernel ----
    Case("stream1", "k_gemm_stream<2, 1, false>", STREAM + STREAM_BETA + MASKED, mnk=(16424, 128, 64), stream=True),
    Case("stream1_two_tiles", "k_gemm_stream<2, 1, false>", STREAM + STREAM_BETA + MASKED, mnk=(16424, 512, 64),
         stream=True),   # 516 tiles over 512 workgroups
    Case("stream1_beta_k128", "k_gemm_stream<2, 1, false>", STREAM_BETA, mnk=(16424, 128, 128), stream=True),
    Case("stream1_masked_k256", "k_gemm_stream<2, 1, false>", MASKED, mnk=(16424, 128, 256), stream=True),
    Case("stream2", "k_gemm_stream<2, 2, false>", STREAM + STREAM_BETA + MASKED, mnk=(16424, 64, 64), stream=True),
    Case("stream2_two_tiles", "k_gemm_stream<2, 2, false>", STREAM + STREAM_BETA + MASKED, mnk=(131330, 64, 64),
         stream=True),   # 514 tiles of 256 rows over 512 workgroups
    Case("stream_conv3x3", "k_gemm_stream<2, 1, true>", STREAM + STREAM_BETA, conv=1,
         geom=(8, 46, 46, 64, 128, 3, 3, 1, 1), stream=True),
    Case("stream_conv1x1_s2", "k_gemm_stream<2, 1, true>", STREAM + STREAM_BETA, conv=1,
         geom=(8, 92, 92, 64, 128, 1, 1, 2, 0), stream=True),
    # ---- row-ring and direct convolutions ----
    *(Case(f"rows3x3_w{w}", f"k_conv3x3_rows<{nf}>", ROWS, conv=1, geom=_rows3x3(w))
      for nf, w in ((1, 11), (2, 20), (3, 40), (4, 64))),
    Case("direct3x3_w70", "k_direct_conv<64, 3, 3>", ROWS, conv=1, geom=_rows3x3(70)),
    *(Case(f"rows3x3_128_w{w}", f"k_conv3x3_rows<{nf}, 128>", ROWS, conv=1, geom=_rows3x3(w, 128))
      for nf, w in ((1, 11), (2, 20))),
    *(Case(f"s2d_w{w}", f"k_conv_s2d_rows<{nf}>", ROWS, conv=1, geom=_s2d(w))
      for nf, w in enumerate((19, 35, 51, 67, 83, 99, 115, 128), 1)),
    Case("direct_stem_w140", "k_direct_conv<16, 4, 4>", ROWS, conv=1, geom=_s2d(140)),
    # ---- weight gradients ----
    Case("wgrad_64_64", "k_wgrad<64, 64, 2>", WGRAD, mnk=(64, 64, 777), splits=3, **_WG,
         route=dict(splits=3, k_per_split=320)),   # ragged last split: 320, 320, 137
    Case("wgrad_64_128", "k_wgrad<64, 128, 1>", WGRAD, mnk=(64, 200, 777), splits=3, **_WG,
         route=dict(splits=3, k_per_split=320)),
    Case("wgrad_128_64", "k_wgrad<128, 64, 4>", WGRAD, mnk=(200, 64, 777), splits=1, **_WG, route=dict(splits=1)),
    Case("wgrad_128_128", "k_wgrad<128, 128, 2>", WGRAD, mnk=(136, 200, 130), splits=2, **_WG,
         route=dict(splits=2, k_per_split=128)),
    Case("wgrad_wperm_c3", "k_wgrad<64, 128, 1>", WPERM, conv=2, ta=1, ws=True, splits=2,
         geom=(2, 9, 10, 8, 64, 3, 3, 1, 1), route=dict(splits=2)),
    Case("wgrad_pp_256", "k_wgrad_pp<256, false>", WGRAD, mnk=(256, 256, 1024), splits=4, **_WG,
         route=dict(splits=4, k_per_split=256)),
    Case("wgrad_pp_128", "k_wgrad_pp<128, false>", WGRAD, mnk=(264, 136, 777), splits=1, **_WG, route=dict(splits=1)),
    Case("wgrad_pp_sw", "k_wgrad_pp<128, true>", WGRAD, mnk=(120, 512, 640), splits=2, **_WG,
         route=dict(splits=2, k_per_split=320)),
    # 4 splits asked; K = 2 x 5 x w pixels in slabs of a multiple of 64: 110 -> 64 + 46, 400 -> 3 x 128 + 16
    Case("wgrad3x3_rows1", "k_wgrad3x3_rows<1>", geom=_rows3x3(11), route=dict(splits=2), **_WGC),
    Case("wgrad3x3_rows2", "k_wgrad3x3_rows<2>", geom=_rows3x3(40), route=dict(splits=4), **_WGC),
    Case("wgrad3x3_rows128", "k_wgrad3x3_rows<1, 128>", geom=_rows3x3(11, 128), route=dict(splits=2), **_WGC),
    # K = 5 (w - 3) pixels in slabs of a multiple of 64: 45 -> 1, 185 -> 3 x 64, 335 -> 3 x 128, 485 -> 4 x 128
    *(Case(f"wgrad_s2d_w{w}", f"k_wgrad_s2d_rows<{nf}>", geom=_s2d(w), route=dict(splits=sp), **_WGC)
      for nf, (w, sp) in enumerate(((12, 1), (40, 3), (70, 3), (100, 4)), 1)),
)

EXCLUDED = {
    "k_gemm_stream<2, 2, true>":
        "routed only under DCA_OPS_STREAM=1 (the 64-column implicit conv stays on the one-tile kernel by default); "
        "tests/_stream_check.py runs it in its forced-mode child process",
    "k_gemm<true, 128>":
        "reachable only through an operand base that is not 16-B aligned, where load_nt issues its 16-B vector loads "
        "at that misaligned address; no test has ever run that on the shared machines and this table does not either",
    "k_gemm<true, 64>":
        "as k_gemm<true, 128>: only a misaligned fp8 operand base routes here",
}
