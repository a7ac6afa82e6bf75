"""GPU: every kernel flavour behind md_gemm_f16 / md_conv_nhwc_f16, each at the smallest shapes that reach its code paths, pinned by the plan
query of the call as it is made (md_gemm_plan_call / md_conv_plan_call through ops.gemm_plan / ops.conv_plan) and held to a floor computed
from the float64 reference alone (tests/gemm_ref.py).  The cases and the three steps of each -- plan, three bit-identical launches with
guarded surroundings, pass rule -- are in tests/gemm_flavours_check.py.  The automatic dispatch runs in this process; MD_GEMM_SP=1 with
each pinned tile and MD_GEMM_SP=0 run that file once in a fresh process each (the knobs are read once per process), one at a time.

Which case asserts which plan code (t = 135 / 134 / 124 / 142 / 132 under MD_GEMM_SP_NT = 5 / 4 / 2 / 42 / 32):
  t, GEMM            sp_gemm_cases(t): ragged tile K = 128 / 192 / 256, below the RESM switch, tile order 11 x 3, wrapped grids (CU limit 8 with
                     19 tiles; the device's count + 44 tiles), bias / row-term set, A / output / residual slices, identity A
  2000 + t, GEMM     sp_gemm_cases(t): K = 64 (MT NT + 1): bias + residual, no bias, + row term, in place, strided residual, A = 0 exact screen,
                     wrapped under the CU limit
  t, conv            sp_conv_cases(t): 13 x 11 x 3 images stride 1 / 2, pad_lo = 0 on an odd and an even side, folded upsample, kw = 1 with 1 and 5
                     frames, channel-slice input and output, wrapped under the CU limit, residual + row term below the RESM switch
  2000 + t, conv     sp_conv_cases(t): residual + row term / in place at the K depth above the switch (9 or 18 K tiles), wrapped
  1134, 1124         transposed_pinned_cases (pins 4, 2): M = 256 / 512, N = 320, with / without bias, ldc_t = M + 8 guarded;
                     1124 also test_transposed_automatic (120 tiles, K = 256; 110 tiles and K = 192 take 303)
  144                geglu_sp_cases (pin 5 process: K = 128 / 640, ragged M = 200, wrapped), test_geglu_automatic (K = 640)
  210, 220           test_streaming_kernels[N-K]: wsgemm_kernel<KS, TPR, RES, RA> -- (320, 320) = <10, 1>, (960, 320) = <10, 2>, (128, 640) =
                     <20, 1>, (640, 640) = <20, 2>, each with none / residual / row term only / both, in place, A and C slices
  230                test_streaming_edges (GEGLU stream; M % 16 = 8 takes 303)
  301                test_occupancy_small (N = 4, 64; GEMM and conv)
  302                test_occupancy_302_conv (Cout = 192, 131072 pixels), test_occupancy_302_gemm (K = 2048, N = 1288), test_geglu_automatic
                     (K = 128, packed N = 1024, M = 32768 + 5), sp_off_cases (MD_GEMM_SP=0)
  303                test_occupancy_small (N = 200, 1288), test_alignment_alone (output base, output pitch, residual base, odd conv pitch,
                     SiLU / ReLU on a conv), SiLU / ReLU in sp_gemm_cases, test_geglu_automatic (K = 128), sp_off_cases
The calls of the CLIP vision tower (mikudance_amd/clip_vision.py), all on gemm_kernel:
  MD_ACT_QUICKGELU   test_quickgelu_automatic: 303 at M = 257, N = 200 (ragged rows, scalar last column group) with bias / none / residual
                     after the activation / row term / column slice / pitch % 8 = 4, and at M = 32768 + 5, K = 128; 301 (N = 64); 302
                     (K = 2048); a conv (303).  test_quickgelu_exact_screen: A = 0 over a bias table from -65504 to 65504 (303 and 301)
  transposed store   test_transposed_ragged_m: M = 257 / 261 (M % 8 = 1 / 5: the scalar tail) into pitch roundup8(M) with a 7.0 guard behind
                     column M and into pitch M (odd); M = 257, N = 320 under pins 4 and 2 (transposed_pinned_cases: 303, M % 256 != 0)
  act outside 0..4   test_unknown_activation_is_refused: MD_ERR_ARG from launch and call query, output untouched (GEGLU on a conv too)
profiles/gemm_flavour_tests.log: floor and measured value of every case on MI355X, the wall time of each test, and the mutations of the
kernels that these cases catch; profiles/clip_kernel_tests.log: the same for the tower's cases."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_flavours_check as C  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert not os.environ.get("MD_GEMM_SP") and not os.environ.get("MD_GEMM_SP_NT"), "the in-process cases are written for the automatic dispatch"
    return torch.device("cuda:0")


_stopped = []          # why no further scripted process is started: one ran into its time limit or died of a signal


def _script(mode, timeout, **env):
    """One fresh process.  After a time limit, an abort or a segmentation fault nothing more is started on the card: the remaining scripted
    tests fail at once, naming the first casualty."""
    assert not _stopped, f"not started: {_stopped[0]}"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_flavours_check.py"), mode], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped.append(f"gemm_flavours_check.py {mode} {env} did not finish in {timeout} s")
        raise
    if r.returncode < 0:
        _stopped.append(f"gemm_flavours_check.py {mode} {env} died of signal {-r.returncode}")
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# Time limits: five times what each process took on the MI355X, interpreter start included (2.6 - 3.5 s; profiles/gemm_flavour_tests.log).
@pytest.mark.parametrize("pin", [5, 4, 2, 42, 32])
def test_sp_tile_under_its_pin(pin):
    _script("pin", 20, MD_GEMM_SP="1", MD_GEMM_SP_NT=str(pin))


def test_gemm_kernel_with_the_sp_kernel_off():
    _script("off", 15, MD_GEMM_SP="0", MD_GEMM_SP_NT="0")


@pytest.mark.parametrize("N,K", [(320, 320), (960, 320), (128, 640), (640, 640)])
def test_streaming_kernels(dev, N, K):
    C.streaming_cases(dev, N, K)


def test_streaming_edges(dev):
    C.streaming_edge_cases(dev)


def test_transposed_automatic(dev):
    C.transposed_auto_cases(dev)


def test_transposed_ragged_m(dev):
    C.transposed_ragged_cases(dev)


def test_geglu_automatic(dev):
    C.geglu_auto_cases(dev)


def test_quickgelu_automatic(dev):
    C.quickgelu_cases(dev)


def test_quickgelu_exact_screen(dev):
    C.quickgelu_screen_cases(dev)


def test_unknown_activation_is_refused(dev):
    C.refused_act_case(dev)


def test_occupancy_small(dev):
    C.occupancy_small_cases(dev)


def test_occupancy_302_conv(dev):
    C.occupancy_302_conv(dev)


def test_occupancy_302_gemm(dev):
    C.occupancy_302_gemm(dev)


def test_alignment_alone(dev):
    C.alignment_cases(dev)
