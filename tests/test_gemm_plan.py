"""The decision table of the dense contractions (csrc/gemm_plan.h): which kernel takes a call and with which launch
parameters -- pure host arithmetic on shapes, strides and pointer alignment, so it is pinned here without a GPU.
tests/sanitize/gemm_plan_driver.cpp prints gemm_plan()'s answer for every case, built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer; the expected lines below are literals, worked out by hand from the launch code as it stood
before the decision had a module of its own (gemm_f32() / gemm_bf16x3_launch() / launch_form() / gemm_bf16x3_w8_launch()).

A line reads: kernel<a_kc,b_kc> terms vec table(B from its fragment table) pro(logue) swz(swizzle) splits kps(k_per_split)
slabs ldc(of what the kernel writes) vecC tiles(tiles_m x tiles_n) grid(x extent).  Unless a case says otherwise: gemm mode
6, RGCN_GEMM_W8 knob 1, one group, 16-byte-aligned pointers, leading dimensions equal to the contiguous extent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_PROLOGUE = "refused: gemm: the A-operand prologue exists in the pre-split-weight NN kernels only"
HEAD = "terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1"      # N = K = 500, mode 6, table

EXPECTED = {
    # NN, M 14541 / 14951 (FB15k-237 / FB15k), wide: 114 x 2 = 228 and 117 x 2 = 234 tiles of 128 x 256 -- one round
    "fwd_14541": "w8<1,0> " + HEAD + " tiles=114x2 grid=228",
    "fwd_14541_bias": "w8<1,0> terms=6 vec=1 table=1 pro=1 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=114x2 grid=228",
    "fwd_14951": "w8<1,0> " + HEAD + " tiles=117x2 grid=234",
    # M 40943 (WN18): 320 x 2 = 640 wide tiles, several rounds -- the 128 x 128 kernel, 320 x 4
    "fwd_40943": "presplit<1,0> " + HEAD + " tiles=320x4 grid=1280",
    "fwd_40943_bias": "presplit<1,0> terms=6 vec=1 table=1 pro=1 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=320x4 grid=1280",
    # wide only for 160 <= tiles <= 256 (N 256: one column tile of the wide kernel, two of the other)
    "wide_t159": "presplit<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=64 slabs=0 ldc=256 vecC=1 tiles=159x2 grid=318",
    "wide_t160": "w8<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=64 slabs=0 ldc=256 vecC=1 tiles=160x1 grid=160",
    "wide_t256": "w8<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=64 slabs=0 ldc=256 vecC=1 tiles=256x1 grid=256",
    "wide_t257": "presplit<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=64 slabs=0 ldc=256 vecC=1 tiles=257x2 grid=514",
    # NT (dH), not wide: 114 x 4 = 456 workgroups; the knob forces (3) or forbids (0) the eight-wavefront kernel
    "nt": "presplit<1,1> " + HEAD + " tiles=114x4 grid=456",
    "nt_knob3": "w8<1,1> " + HEAD + " tiles=114x2 grid=228",
    "nt_knob0": "presplit<1,1> " + HEAD + " tiles=114x4 grid=456",
    "nt_wide_knob0": "presplit<1,1> " + HEAD + " tiles=114x4 grid=456",
    "fwd_14541_knob0": "presplit<1,0> " + HEAD + " tiles=114x4 grid=456",
    # TN (dW): ceil(14541 / 8) = 1818 -> 1824 per slice, 8 slices, slabs of leading dimension N
    "tn_split8": "staged<0,0> terms=6 vec=1 table=0 pro=0 swz=1 splits=8 kps=1824 slabs=1 ldc=500 vecC=1 tiles=4x4 grid=128",
    "tt": "refused: gemm TT form not instantiated",
    "empty_m0": "none",
    "empty_n0": "none",
    "empty_m_negative": "none",      # (a TT call with a bias: the empty shape is looked at first)
    # mode 0: the fp32 MFMA whatever the batch offers and the knob says
    "mode0": "f32<1,0> terms=0 vec=1 table=0 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=114x4 grid=456",
    "mode0_tn_split8": "f32<0,0> terms=0 vec=1 table=0 pro=0 swz=1 splits=8 kps=1824 slabs=1 ldc=500 vecC=1 tiles=4x4 grid=128",
    "mode0_bias": NO_PROLOGUE,
    "mode9": "w8<1,0> terms=9 vec=1 table=1 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=114x2 grid=228",
    "mode9_bias": "w8<1,0> terms=9 vec=1 table=1 pro=1 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=114x2 grid=228",
    # mode 3: never the eight-wavefront kernel, never the prologue
    "mode3_knob3": "presplit<1,0> terms=3 vec=1 table=1 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=114x4 grid=456",
    "mode3_bias": NO_PROLOGUE,
    # the prologue's bias copy holds 127 k-tiles
    "pro_k2032": "presplit<1,0> terms=6 vec=1 table=1 pro=1 swz=1 splits=1 kps=2032 slabs=0 ldc=128 vecC=1 tiles=2x1 grid=2",
    "pro_k2036": NO_PROLOGUE,
    "pro_nt": NO_PROLOGUE,
    "pro_split2": NO_PROLOGUE,
    "pro_limit_on_k": NO_PROLOGUE,
    "pro_no_table": NO_PROLOGUE,
    # operands that 16-byte loads cannot take: the table is ignored, the staged kernel loads dwords
    "a_off4": "staged<1,0> terms=6 vec=0 table=0 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=128 vecC=1 tiles=2x1 grid=2",
    "a_off4_bias": NO_PROLOGUE,
    "lda502": "staged<1,0> terms=6 vec=0 table=0 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=128 vecC=1 tiles=2x1 grid=2",
    "k502": "staged<1,0> terms=6 vec=0 table=0 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=128 vecC=1 tiles=2x1 grid=2",
    # B behind its table is never read: its width and alignment do not matter -- unless the CALLER asked for a split over K
    "n5_b_off4": "presplit<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=5 vecC=0 tiles=2x1 grid=2",
    "n5_b_off4_split4_k16": "staged<1,0> terms=6 vec=0 table=0 pro=0 swz=1 splits=1 kps=16 slabs=0 ldc=5 vecC=0 tiles=2x1 grid=2",
    # a device-side row limit: swizzle 2, ceil(9 / 8) * 8 row panels x the column tiles; a wide request stays wide
    "groups_row_limit": "w8<1,0> terms=6 vec=1 table=1 pro=0 swz=2 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=9x2 grid=32",
    "groups_row_limit_strideA_odd": "staged<1,0> terms=6 vec=0 table=0 pro=0 swz=2 splits=1 kps=512 slabs=0 ldc=500 vecC=1 tiles=9x4 grid=64",
    # groups whose products lie an odd number of floats apart: no 16-byte stores
    "groups_row_limit_strideC_odd": "w8<1,0> terms=6 vec=1 table=1 pro=0 swz=2 splits=1 kps=512 slabs=0 ldc=500 vecC=0 tiles=9x2 grid=32",
    # a row limit with a split over K is refused: tiles beyond the extent write no slab, and the reduce sums whole slabs
    "row_limit_split8": "refused: gemm: a row limit cannot be combined with a split over K",
    "limit_on_k_split8": "staged<0,0> terms=6 vec=1 table=0 pro=0 swz=1 splits=8 kps=1824 slabs=1 ldc=500 vecC=1 tiles=4x4 grid=128",
    # a limit on K never reaches the eight-wavefront kernel (it reads the limit as a row limit)
    "limit_on_k_knob3": "presplit<1,0> terms=6 vec=1 table=1 pro=0 swz=1 splits=1 kps=512 slabs=0 ldc=128 vecC=1 tiles=2x1 grid=2",
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gemm_plan_table_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "gemm_plan_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "gemm_plan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "gemm_plan_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert len(got) == len(lines) - 1, "a case name printed twice"
    wrong = {k: (got.get(k), v) for k, v in EXPECTED.items() if got.get(k) != v}
    assert not wrong, "\n".join("%s:\n  got      %s\n  expected %s" % (k, g, e) for k, (g, e) in wrong.items())
    assert set(got) == set(EXPECTED), sorted(set(got) ^ set(EXPECTED))
