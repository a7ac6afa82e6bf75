"""TEST INFRASTRUCTURE shared by the CPU tests of the sampling loop (DPM-Solver++, guidance rescale, video-to-video, window fusion, FreeInit, APG,
PAG, K / V downsampling, SEG): the small models and inputs, a UNet stand-in that counts calls, the two parity measures, the three-rank gloo harness
(worker_setup installs every emulated operator) and the script's input tree.  The operators themselves are emulated in tests/fake_ops.py and, beside
their feature's restatement, in tests/*_ref.py; fake_ops.install / install_process install all of them."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mikudance_amd.selftest import SCHED_KWARGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()))


@pytest.fixture(scope="module")
def small_cpu():
    """(ref, den, ref_sd, den_sd) at reduced width on the CPU, once per test module that imports this fixture."""
    from mikudance_amd.selftest import build_models
    return build_models(device="cpu")


def small_inputs(frames, seed):
    """(latents, ref_latents, embeds) at 16 x 16, fp16-representable fp32 (the oracle takes them as they are, the pipeline after .half())."""
    from mikudance_amd.synth import synth_inputs
    return tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


def zero_inputs():
    """The smallest well-formed denoise() arguments, for refusals that must come before any model runs."""
    return torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16), torch.zeros(1, 2, 22, 2, 2, dtype=torch.float16), torch.zeros(2, 5, 64, dtype=torch.float16)


class CountingUNet:
    """Answers every method and counts the calls: a refusal is in time if the count is still 0."""

    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def f(*a, **k):
            self.calls += 1
        return f


# ---- window parallelism over gloo
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def worker_setup(rank, world, port):
    """First thing in a spawned worker: the import path, the rendezvous environment, the emulated operators, gloo."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import fake_ops
    from mikudance_amd import dp
    fake_ops.install_process()
    dp.init(backend="gloo")


def run_world(world, worker, *args):
    """Spawn worker(rank, world, port, queue, *args) on `world` ranks; -> what rank 0 put on the queue.  Every rank must exit with 0."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


# ---- the drop-in script
def script_tree(tmp_path, frames=2, size=32):
    """Configs and input media of mikudance_amd.inference_video under tmp_path -> (path of the YAML, size)."""
    import yaml
    from PIL import Image
    from mikudance_amd import io_utils as U
    os.makedirs(tmp_path / "inputs")
    rng = np.random.default_rng(0)
    img = lambda: Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8))
    img().save(tmp_path / "inputs" / "ref.png")
    img().save(tmp_path / "inputs" / "skel.png")
    U.save_videos_from_pil([img() for _ in range(frames)], str(tmp_path / "inputs" / "pose.mp4"), fps=12)
    yaml.safe_dump({"noise_scheduler_kwargs": SCHED_KWARGS}, open(tmp_path / "infer.yaml", "w"))
    yaml.safe_dump({"inference_config": str(tmp_path / "infer.yaml"), "weight_dtype": "fp16", "ref_image_path": str(tmp_path / "inputs" / "ref.png"),
                    "ref_skel_path": str(tmp_path / "inputs" / "skel.png"), "ref_depth_path": "None", "tgt_pose_path": str(tmp_path / "inputs" / "pose.mp4"),
                    "tgt_face_path": "None", "tgt_hand_path": "None", "tgt_w2c_path": "None", "tgt_c2w_path": "None"}, open(tmp_path / "cfg.yaml", "w"))
    return str(tmp_path / "cfg.yaml"), size


def fake_pipeline_builder(IV):
    """A stand-in for inference_video.build_pipeline: the real pipeline class and scheduler on the duck-typed VAE / CLIP of fake_ops, no UNets."""
    import types
    import fake_ops
    import mikudance_amd as M

    def build(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim"):
        pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None,
                                        denoising_unet=types.SimpleNamespace(in_channels=4), scheduler=IV.build_scheduler(infer_config, sampler))
        pipe._device = torch.device("cpu")
        return pipe
    return build
