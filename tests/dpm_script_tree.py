"""TEST INFRASTRUCTURE: the synthetic `pretrained_weights/` tree + YAML configs + input media of tests/test_inference_script_gpu.py
(same layout, same cheap seeded weights), built under a temporary directory for further runs of the drop-in script."""
import json
import os

import numpy as np
import torch
from PIL import Image
from safetensors.torch import save_file

import mikudance_amd as M
from mikudance_amd import io_utils as U
from mikudance_amd.selftest import MM_KWARGS, SCHED_KWARGS
from test_inference_script_gpu import cheap_state_dict

UNET_CFG = {"_class_name": "UNet2DConditionModel", "act_fn": "silu", "attention_head_dim": 8, "block_out_channels": [320, 640, 1280, 1280],
            "center_input_sample": False, "cross_attention_dim": 768, "downsample_padding": 1, "flip_sin_to_cos": True, "freq_shift": 0,
            "in_channels": 4, "layers_per_block": 2, "mid_block_scale_factor": 1, "norm_eps": 1e-05, "norm_num_groups": 32,
            "out_channels": 4, "sample_size": 64,
            "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
            "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"]}
VAE_CFG = {"_class_name": "AutoencoderKL", "in_channels": 3, "out_channels": 3, "block_out_channels": [64, 64, 128, 128], "latent_channels": 4,
           "layers_per_block": 2, "norm_num_groups": 32, "act_fn": "silu", "scaling_factor": 0.18215, "sample_size": 256}
CLIP_CFG = {"hidden_size": 128, "intermediate_size": 256, "num_hidden_layers": 2, "num_attention_heads": 4, "image_size": 224, "patch_size": 56,
            "projection_dim": 768, "hidden_act": "quick_gelu", "model_type": "clip_vision_model"}


def make_tree(tmp_path, golden_dir, frames=2, width=64, height=64):
    """-> (path of the inference YAML, W, H, frames)."""
    import yaml
    root = tmp_path / "pretrained_weights"
    sd15, vae_d, enc_d = root / "stable-diffusion-v1-5" / "unet", root / "sd-vae-ft-mse", root / "image_encoder"
    for d in (sd15, vae_d, enc_d, tmp_path / "configs", tmp_path / "inputs"):
        os.makedirs(d)
    json.dump(UNET_CFG, open(sd15 / "config.json", "w"))
    den_sd = cheap_state_dict(lambda: M.UNet3DConditionModel(sample_size=64, cross_attention_dim=768, **MM_KWARGS), 1)
    save_file({k: v for k, v in den_sd.items() if "motion_modules" not in k}, str(sd15 / "diffusion_pytorch_model.safetensors"))
    torch.save({k: v for k, v in den_sd.items() if "motion_modules" in k}, root / "motion_module.pth")
    torch.save({k: v for k, v in den_sd.items() if k.startswith("conv_in.")}, root / "denoising_unet.pth")
    del den_sd
    torch.save(cheap_state_dict(lambda: M.UNet2DConditionModel(cross_attention_dim=768), 2), root / "reference_unet.pth")
    json.dump(VAE_CFG, open(vae_d / "config.json", "w"))
    save_file(cheap_state_dict(lambda: M.AutoencoderKL(**VAE_CFG), 3), str(vae_d / "diffusion_pytorch_model.safetensors"))
    json.dump(CLIP_CFG, open(enc_d / "config.json", "w"))
    save_file(cheap_state_dict(lambda: M.CLIPVisionModelWithProjection(CLIP_CFG), 4), str(enc_d / "model.safetensors"))
    rng = np.random.default_rng(0)
    img = lambda: Image.fromarray(np.kron(rng.integers(0, 255, (height // 8 + 2, width // 8 + 1, 3), dtype=np.uint8),
                                          np.ones((8, 8, 1), dtype=np.uint8)))
    img().save(tmp_path / "inputs" / "img-char.jpg")
    img().save(tmp_path / "inputs" / "skel-img-char.jpg")
    U.save_videos_from_pil([img() for _ in range(frames)], str(tmp_path / "inputs" / "pose-demo.mp4"), fps=12)
    z = np.load(os.path.join(golden_dir, "g2_scene_motion.npz"))
    np.save(tmp_path / "inputs" / "w2c.npy", z["w2c"][:frames])
    np.save(tmp_path / "inputs" / "c2w.npy", z["c2w"][:frames])
    np.save(tmp_path / "inputs" / "depth.npy", np.kron(z["depth"], np.ones((1, 4, 4))))
    yaml.safe_dump({"unet_additional_kwargs": MM_KWARGS, "noise_scheduler_kwargs": SCHED_KWARGS, "sampler": "DDIM"},
                   open(tmp_path / "configs" / "mikudance_config.yaml", "w"))
    cfg = tmp_path / "configs" / "inference_video.yaml"
    yaml.safe_dump({"pretrained_base_model_path": str(root / "stable-diffusion-v1-5"), "pretrained_vae_path": str(vae_d),
                    "pretrained_temporal_vae_path": str(root / "vae_temporal_decoder"), "image_encoder_path": str(enc_d),
                    "denoising_unet_path": str(root / "denoising_unet.pth"), "reference_unet_path": str(root / "reference_unet.pth"),
                    "motion_module_path": str(root / "motion_module.pth"), "inference_config": str(tmp_path / "configs" / "mikudance_config.yaml"),
                    "weight_dtype": "fp16", "ref_image_path": str(tmp_path / "inputs" / "img-char.jpg"),
                    "ref_skel_path": str(tmp_path / "inputs" / "skel-img-char.jpg"), "ref_depth_path": str(tmp_path / "inputs" / "depth.npy"),
                    "tgt_pose_path": str(tmp_path / "inputs" / "pose-demo.mp4"), "tgt_face_path": "None", "tgt_hand_path": "None",
                    "tgt_w2c_path": str(tmp_path / "inputs" / "w2c.npy"), "tgt_c2w_path": str(tmp_path / "inputs" / "c2w.npy")},
                   open(cfg, "w"))
    return str(cfg), width, height, frames
