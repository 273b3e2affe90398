"""HIP building blocks for training arbitrary CNNs and vision transformers on MI355X (gfx950).

The NetResDeep fast path is the fused engine (``runtime/engine.py``); this layer is what any other model (and
NetResDeep outside the engine) trains on: MFMA GEMM (bf16 / fp8 e4m3), im2col convolution, BatchNorm with
fused ReLU / residual, grouped and depthwise 3x3 convolution, squeeze-and-excitation, fused multi-head
self-attention (``attention``), LayerNorm fused with the residual add (``layer_norm``), GELU (``gelu``,
``linear(gelu=True)``), pooling, ROI-align, cross-entropy, flat SGD and Adam, fp8 quantisation -- see
``functional.py``.
"""
from .functional import (SELink, adam_step_, attention, batch_norm_act, conv2d, conv_bn_act, cross_entropy,  # noqa: F401
                         fp8_alpha, gconv_ok, gelu, gemm, global_avg_pool, layer_norm, linear, max_pool2d,
                         quantize_fp8, roi_align, se_scale, se_squeeze, sgd_step_)
from .models import OpsModel  # noqa: F401
