#!/usr/bin/env python
"""The encoder's weight products on their own, through librgcn_devtools.so: mean time of one product of the staged
kernel (k_gemm_bf16x3, B split on the fly) and of both kernels for a pre-split weight -- k_gemm_bf16x3<.., B_PRE>
(128x128, 4 wavefronts; RGCN_GEMM_W8=0) and k_gemm_w8 (128x256, 8 wavefronts, LDS-DMA; RGCN_GEMM_W8=3) --
interleaved, ROUNDS times per shape, with a bitwise comparison of the two pre-split results.
    python tools/gemm_time.py [gemm mode, default 6]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relationprediction_amd import _native  # noqa: E402

SHAPES = [("self_fwd  H.W", 14541, 500, 500, False), ("self_dh   dS.W^T", 14541, 500, 500, True),
          ("basis fwd b2 (5370 rows)", 5370, 500, 1000, False), ("basis dz b2 (7082 rows)", 7082, 1000, 500, True),
          ("wn18 self_fwd", 40943, 500, 500, False)]
ROUNDS = int(os.environ.get("ROUNDS", "3"))
mode = int(sys.argv[1]) if len(sys.argv) > 1 else 6
rng = np.random.RandomState(0)
with _native.Engine(16, 2, 8, 1, "block", 2, max_edges=4, devtools=True) as eng:
    eng.set_gemm_mode(mode)
    for name, M, N, K, tb in SHAPES:
        A = rng.randn(M, K).astype(np.float32)
        B = rng.randn(K, N).astype(np.float32)
        Bop = np.ascontiguousarray(B.T) if tb else B
        times = {"staged": [], "pre-split 128x128": [], "k_gemm_w8": []}
        for rep in range(ROUNDS):
            times["staged"].append(eng.debug_gemm_time(A, Bop, trans_b=tb, split_k=1, iters=50) * 1e3)
            outs = []
            for key, code in (("pre-split 128x128", "0"), ("k_gemm_w8", "3")):
                os.environ["RGCN_GEMM_W8"] = code
                out, ms = eng.debug_gemm_presplit(A, Bop, trans_b=tb, iters=50)
                times[key].append(ms * 1e3)
                outs.append(out)
            if not np.array_equal(outs[0], outs[1]):
                print("   !! the two pre-split kernels differ: max |d| %.3g at %d entries" % (
                    float(np.abs(outs[0] - outs[1]).max()), int((outs[0] != outs[1]).sum())))
        print("mode %d %-28s " % (mode, name) + "   ".join(
            "%s %s us" % (k, "/".join("%.1f" % t for t in v)) for k, v in times.items()), flush=True)
