#!/usr/bin/env python
"""A few launches of each GEMM kernel, for rocprofv3 --pmc (tools/gpu_pmc.sh gemm k_gemm gemm): the three self-loop
forms (staged kernel), then H.W_self with a pre-split weight on both of its kernels (RGCN_GEMM_W8 = 0: 128x128,
3: k_gemm_w8)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relationprediction_amd import _native  # noqa: E402

V, d = 14541, 500
rng = np.random.RandomState(0)
H = np.maximum(rng.randn(V, d), 0).astype(np.float32)
W = rng.randn(d, d).astype(np.float32)
D = rng.randn(V, d).astype(np.float32)
with _native.Engine(V, 4, d, 1, "block", 100, max_edges=16, devtools=True) as eng:
    print("NN", eng.debug_gemm_time(H, W, iters=5))
    print("NT", eng.debug_gemm_time(D, W, trans_b=True, iters=5))
    print("TN", eng.debug_gemm_time(H, D, trans_a=True, iters=5))
    for code in ("0", "3"):
        os.environ["RGCN_GEMM_W8"] = code
        _, ms = eng.debug_gemm_presplit(H, W, iters=10)
        print("pre-split, RGCN_GEMM_W8=%s: %.1f us" % (code, ms * 1e3))
