"""ops: general-purpose MI355X layer kernels (HIP, gfx950) as autograd functions, and model forwards on them.

The NetResDeep fast path is the fused engine (``runtime/engine.py``); this layer is what any other model (and
NetResDeep outside the engine) trains on: MFMA GEMM (bf16 / fp8 e4m3), im2col convolution, BatchNorm with
fused ReLU / residual, grouped and depthwise 3x3 convolution, squeeze-and-excitation, pooling, ROI-align,
cross-entropy, flat SGD and Adam, fp8 quantisation -- see ``functional.py``.
"""
from .functional import (SELink, adam_step_, batch_norm_act, conv2d, conv_bn_act, cross_entropy, fp8_alpha,  # noqa: F401
                         gconv_ok, gemm, global_avg_pool, linear, max_pool2d, quantize_fp8, roi_align, se_scale,
                         se_squeeze, sgd_step_)
from .models import OpsModel  # noqa: F401
