"""CPU: video-to-video sampling (init_latents= / video= and strength=) -- the schedulers' get_timesteps against a restatement of diffusers'
img2img rule, DPM-Solver++'s set_begin_index table against the float64 restatement of tests/dpmpp_ref.py, every argument check, the host
loop of MikuDanceVideoPipeline.denoise() on emulated operators against the oracle on a truncated, pre-noised schedule (tests/v2v_ref.py),
__call__'s video= keyword and the script's --init_video / --strength."""
import math
import os
import types

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import v2v_ref as V
from loop_helpers import CountingUNet, fake_pipeline_builder, rel_l2, script_tree, small_cpu, small_inputs, zero_inputs  # noqa: F401 (small_cpu: fixture)

MODES = [dict(), dict(algorithm_type="sde-dpmsolver++"), dict(solver_type="heun"), dict(algorithm_type="sde-dpmsolver++", solver_type="heun")]
MODE_IDS = ["2m-midpoint", "2m-sde-midpoint", "2m-heun", "2m-sde-heun"]
STRENGTHS = [1.0, 0.5, 0.33, 0.05, 0.57, 0.3, 0.29, 0.7, 0.1, 0.99, 0.999999, 1e-9, 0.15, 0.6, 0.9]


def _dpm(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


# ---- 1. get_timesteps: diffusers' img2img rule, literally
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_get_timesteps_matches_restatement(make):
    s = make()
    for n in range(1, 51):
        for strength in STRENGTHS:
            s.set_timesteps(n)
            full = s.timesteps.tolist()
            ts, kept = s.get_timesteps(n, strength)
            want = V.kept_steps(n, strength)
            assert kept == want and ts.tolist() == full[n - want:], (n, strength, kept, want)
            if isinstance(s, M.DPMSolverMultistepScheduler):
                assert s.begin_index == (n - want if want else 0), (n, strength)


def test_get_timesteps_keeps_the_float_product():
    s = _ddim()
    s.set_timesteps(100)
    assert s.get_timesteps(100, 0.57)[1] == 56                     # 0.57 * 100 = 56.99999999999999
    s.set_timesteps(10)
    ts, kept = s.get_timesteps(10, 0.5)
    assert kept == 5 and ts.tolist() == [499, 399, 299, 199, 99]
    s.set_timesteps(3)
    assert s.get_timesteps(3, 0.33)[1] == 0                        # no step left: the pipeline refuses it
    with pytest.raises(ValueError, match="set_timesteps"):
        s.get_timesteps(4, 0.5)                                    # the schedule has 3 steps


def test_ddim_step_coefficients_keep_the_full_step_size():
    s = _ddim()
    s.set_timesteps(10)
    full = [s.step_coefficients(t) for t in s.timesteps.tolist()]
    ts, _ = s.get_timesteps(10, 0.3)
    assert [s.step_coefficients(t) for t in ts.tolist()] == full[7:]
    assert s.step_coefficients(ts[0])[1] == float(s.alphas_cumprod[int(ts[0]) - 100])


# ---- 2. DPM-Solver++ set_begin_index
@pytest.mark.parametrize("n", [4, 10, 20])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_set_begin_index_table(n, mode):
    algo, solver = mode.get("algorithm_type", "dpmsolver++"), mode.get("solver_type", "midpoint")
    s = _dpm(**mode)
    s.set_timesteps(n)
    full = [s.multistep_coefficients(i) for i in range(n)]
    first = R.coefficients(n, 1, algo, solver)
    for begin in range(n):
        s.set_begin_index(begin)
        assert s.begin_index == begin
        got = [s.multistep_coefficients(i) for i in range(n)]
        for i in range(n):
            if i != begin:
                assert got[i] == full[i], (begin, i)
        assert got[begin][4] == 0.0 and all(math.isfinite(v) for v in got[begin])
        assert np.allclose(got[begin], first[begin], rtol=1e-12, atol=1e-12), (begin, got[begin], first[begin])
        assert got[-1][2:] == full[-1][2:]                          # the final-step rule stays keyed on the full schedule
    s.set_timesteps(n)
    assert s.begin_index == 0 and [s.multistep_coefficients(i) for i in range(n)] == full


def test_set_begin_index_refuses_bad_indices():
    s = _dpm()
    with pytest.raises(ValueError, match="set_timesteps"):
        s.set_begin_index(0)
    s.set_timesteps(5)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="begin_index"):
            s.set_begin_index(bad)


# ---- 3. argument checks, raised on CPU tensors before anything runs
BAD = [  # (strength, init_latents shape or None, steps, message)
    (float("nan"), (1, 4, 2, 2, 2), 4, "strength must be"), (float("inf"), (1, 4, 2, 2, 2), 4, "strength must be"),
    (0.0, (1, 4, 2, 2, 2), 4, "strength must be"), (-0.5, (1, 4, 2, 2, 2), 4, "strength must be"), (1.5, (1, 4, 2, 2, 2), 4, "strength must be"),
    (1.0000001, None, 4, "strength must be"), (0.5, None, 4, "needs a clip"), (0.5, (1, 4, 3, 2, 2), 4, "do not match"),
    (1.0, (4, 2, 2, 2), 4, "do not match"), (0.33, (1, 4, 2, 2, 2), 3, "After adjusting the num_inference_steps"),
    (0.05, (1, 4, 2, 2, 2), 10, "After adjusting the num_inference_steps")]


@pytest.mark.parametrize("strength,shape,steps,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(strength, shape, steps, msg, make):
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    init = None if shape is None else torch.zeros(shape, dtype=torch.float16)
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), steps, 3.5, init_latents=init, strength=strength)
    assert refu.calls == 0 and den.calls == 0


# ---- 4. the host loop on emulated operators
def _inputs(frames, seed):
    lat, rl, emb = (t.half() for t in small_inputs(frames, seed))
    x0 = (torch.randn(lat.shape, generator=torch.Generator().manual_seed(seed + 1)) * 0.8).half()
    return lat, rl, emb, x0


@pytest.mark.parametrize("sampler,strength", [("ddim", 0.5), ("2m", 0.5), ("2m", 0.3), ("2m-sde", 0.5)])
def test_host_loop_matches_oracle(monkeypatch, small_cpu, sampler, strength):
    from oracle import cpu_ref as O
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb, x0 = _inputs(4, 21)
    algo = "sde-dpmsolver++" if sampler == "2m-sde" else "dpmsolver++"
    sch = _ddim() if sampler == "ddim" else _dpm(algorithm_type=algo)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    steps = []
    out = pipe.denoise(lat, rl, emb, 8, 3.5, generator=torch.Generator().manual_seed(5), init_latents=x0, strength=strength,
                       callback=lambda i, t, x: steps.append((i, t)))
    kept = V.kept_steps(8, strength)
    assert steps == list(enumerate([999, 874, 749, 624, 499, 374, 249, 124][8 - kept:]))
    tail = fake_ops.tail_calls()
    a, b = sch.noise_coefficients(steps[0][1])
    assert tail[0] == ("add_noise", dict(a=a, b=b, keywords=()))
    if sampler != "ddim":
        assert fake_ops.tail_calls("cfg_multistep_step")[0][1]["c_m1"] == 0.0      # the first kept step is order 1
    inner = O.DDIM() if sampler == "ddim" else R.Restated(2, algo, "midpoint", generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = V.denoise_loop(ref_sd, den_sd, lat.float(), rl.float(), emb.float(), 8, x0.float(), strength, scheduler=inner,
                              guidance_scale=3.5, reduced=True)
        plain = O.denoise_loop(ref_sd, den_sd, lat.float(), rl.float(), emb.float(), 8, guidance_scale=3.5, reduced=True)
    r = rel_l2(out.float(), want)
    print(f"\nV2V_HOST_LOOP {sampler} strength {strength} rel_l2 {r:.3e} (from the plain loop {rel_l2(want, plain):.3e})")
    assert torch.isfinite(out).all() and r < 2e-2 and rel_l2(want, plain) > 0.1, r


@pytest.mark.parametrize("sampler", ["ddim", "ddim-eta", "2m", "2m-sde"])
def test_strength_1_equals_the_plain_loop(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb, x0 = _inputs(4, 31)
    x0[0, 0, 0, 0, 0], x0[0, 1, 1, 1, 1] = float("nan"), float("inf")
    sch = _ddim() if sampler.startswith("ddim") else _dpm(algorithm_type="sde-dpmsolver++" if sampler == "2m-sde" else "dpmsolver++")
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    eta = 0.5 if sampler == "ddim-eta" else 0.0
    a = pipe.denoise(lat, rl, emb, 3, 3.5, eta=eta, generator=torch.Generator().manual_seed(9))
    assert not fake_ops.tail_calls("add_noise")                        # no new call without init_latents
    b = pipe.denoise(lat, rl, emb, 3, 3.5, eta=eta, generator=torch.Generator().manual_seed(9), init_latents=x0, strength=1.0)
    assert [d for _, d in fake_ops.tail_calls("add_noise")] == [dict(a=0.0, b=1.0, keywords=())]
    assert torch.equal(a, b)


# ---- 5. __call__(video=, strength=)
def _frames(n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return [Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8)) for _ in range(n)]


def test_call_encodes_video_and_forwards_it(monkeypatch):
    """MikuDanceVideoPipeline.__call__ and Pose2VideoPipeline.__call__: the frames are encoded like the reference image and reach denoise()
    as init_latents (1, 4, F, h, w) with strength; the noise is the generator's first draw, as without video."""
    from mikudance_amd.pipeline_mikudance import _pil_to_tensor
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((latents.clone(), kw.get("init_latents"), kw.get("strength")))
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img, = _frames(1, 32, 1)
    video = _frames(3, 40, 2)
    den = types.SimpleNamespace(in_channels=4)
    vae = fake_ops.FakeVAE()
    want = torch.cat([vae.encode(_pil_to_tensor(im, 32, 32, True)).latent_dist.mean * 0.18215 for im in video]).permute(1, 0, 2, 3)[None]
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        pipe = cls(vae=vae, image_encoder=fake_ops.FakeCLIP(), reference_unet=None, denoising_unet=den, scheduler=_ddim())
        motion = np.zeros((3, 2, 4, 4), dtype=np.float32)
        args = (img, img, [img] * 3, [img] * 3, [img] * 3, motion, 32, 32, 3, 4, 3.5)
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), video=video, strength=0.5)
        pipe(*args, generator=torch.Generator().manual_seed(0), video=video)
        (n0, i0, s0), (n1, i1, s1), (n2, i2, s2) = seen
        assert i0 is None and s0 == 1.0
        assert torch.equal(n0, n1) and torch.equal(n0, n2)           # the generator stream does not change
        assert i1.shape == (1, 4, 3, 4, 4) and torch.allclose(i1.float(), want.float(), atol=1e-6) and s1 == 0.5
        assert torch.equal(i1, i2) and s2 == 1.0
        with pytest.raises(ValueError, match="video has 2 frames"):
            pipe(*args, generator=torch.Generator().manual_seed(0), video=video[:2], strength=0.5)
        with pytest.raises(ValueError, match="needs a clip"):
            pipe(*args, generator=torch.Generator().manual_seed(0), strength=0.5)
        with pytest.raises(ValueError, match="strength must be"):
            pipe(*args, generator=torch.Generator().manual_seed(0), video=video, strength=0.0)
        assert len(seen) == 3


# ---- 6. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert a.strength == 1.0 and a.init_video is None
    a = IV.parse_args(["--init_video", "clip.mp4", "--strength", "0.5"])
    assert a.strength == 0.5 and a.init_video == "clip.mp4"
    assert IV.parse_args(["--init_video", "clip.mp4"]).strength == 1.0
    for argv in (["--strength", "0.5"], ["--strength", "0.999"], ["--strength", "high", "--init_video", "x.mp4"]):
        with pytest.raises(SystemExit):
            IV.parse_args(argv)


def test_script_init_video_reaches_denoise_and_frame_counts_must_match(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    from mikudance_amd import io_utils as U
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((kw["init_latents"], kw["strength"]))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    init = str(tmp_path / "inputs" / "init.mp4")
    U.save_videos_from_pil(_frames(2, size, 7), init, fps=12)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "4", "--output_dir", str(tmp_path / "out")]
    out = IV.main(base + ["--init_video", init, "--strength", "0.5"])
    assert os.path.exists(out) and len(seen) == 1
    assert seen[0][0].shape == (1, 4, 2, size // 8, size // 8) and seen[0][1] == 0.5
    IV.main(base)
    assert seen[1] == (None, 1.0)
    three = str(tmp_path / "inputs" / "three.mp4")
    U.save_videos_from_pil(_frames(3, size, 8), three, fps=12)
    with pytest.raises(ValueError, match="3 frames, the pose video 2"):
        IV.main(base + ["--init_video", three, "--strength", "0.5"])
    assert len(seen) == 2
