"""DDIMScheduler -- host-side mirror of diffusers==0.24.0 DDIMScheduler for the configuration MikuDance uses
(reference configs/inference/mikudance_config.yaml:24-33; constructed at scripts/inference_video.py:101-102):
linear betas rescaled to zero terminal SNR, v-prediction, trailing timestep spacing; eta = 0 (the script's default) or eta > 0.
The table is 1000 fp32 scalars on the host; the per-step arithmetic on the latents is the HIP kernel
md_cfg_ddim_step (fused with window averaging and classifier-free guidance).

DPMSolverMultistepScheduler -- DPM-Solver++ (Lu et al., arXiv 2211.01095) orders 1 / 2, ODE or SDE, restated on the same discrete
table (not pinned to a diffusers version): every step is ONE linear update with host scalars, run by md_cfg_multistep_step.

UniPCMultistepScheduler -- UniPC (Zhao et al., arXiv 2302.04867; diffusers' UniPCMultistepScheduler in its data-prediction form), orders
1 - 3, B(h) = h (bh1) or expm1(h) (bh2), restated on the same table: every step is ONE fused correct-then-predict update whose weights are
host scalars, run by md_cfg_unipc_step.

All take diffusers' video-to-video / img2img entry points: get_timesteps(num_inference_steps, strength) keeps the tail of the schedule and
add_noise(original_samples, noise, timesteps) noises a clean latent to its first timestep (md_add_noise_f16)."""
import inspect
import math
from dataclasses import dataclass

import numpy as np
import torch


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers.utils.torch_utils.randn_tensor for one generator: the draw happens on the GENERATOR's device (a CPU generator ->
    CPU draw, then moved: what scripts/inference_video.py's torch.manual_seed generator gives) so that results do not depend
    on where the model lives."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    gdev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)


def _linear_betas(beta_start, beta_end, num_train_timesteps, rescale_betas_zero_snr):
    """Linear betas in fp32, optionally rescaled to zero terminal SNR (alphas_cumprod[-1] == 0 exactly)."""
    betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    if rescale_betas_zero_snr:
        s = torch.cumprod(1.0 - betas, dim=0).sqrt()
        s0, sT = s[0].clone(), s[-1].clone()
        s = (s - sT) * (s0 / (s0 - sT))
        ab = s ** 2
        betas = 1 - torch.cat([ab[0:1], ab[1:] / ab[:-1]])
    return betas


class _StrengthMixin:
    """The video-to-video start shared by the schedulers (diffusers img2img / video2video pipelines): keep only the tail of the schedule
    and noise the clean latent to its first timestep."""

    def get_timesteps(self, num_inference_steps: int, strength: float):
        """diffusers StableDiffusionImg2ImgPipeline.get_timesteps, literally: init = min(int(N * strength), N), t_start = max(N - init, 0),
        the kept list is timesteps[t_start * order:] (and a scheduler with set_begin_index is told t_start * order).  The float product and
        int() stay as diffusers writes them (0.57 * 100 -> 56 steps).  Call after set_timesteps(num_inference_steps).
        Returns (timesteps, num_inference_steps - t_start)."""
        if self.num_inference_steps != num_inference_steps:
            raise ValueError(f"get_timesteps({num_inference_steps}, ...): call set_timesteps({num_inference_steps}) first "
                             f"(the schedule has {self.num_inference_steps} steps)")
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        timesteps = self.timesteps[t_start * self.order:]
        if hasattr(self, "set_begin_index") and len(timesteps):
            self.set_begin_index(t_start * self.order)
        return timesteps, num_inference_steps - t_start

    def noise_coefficients(self, timestep):
        """(sqrt(abar_t), sqrt(1 - abar_t)) as Python floats, computed in float64 from the fp32 table: the (a, b) of md_add_noise_f16."""
        abar = float(self.alphas_cumprod[int(timestep)])
        return math.sqrt(abar), math.sqrt(1.0 - abar)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' add_noise(original_samples, noise, timesteps) = sqrt(abar_t) x0 + sqrt(1 - abar_t) noise on GPU tensors of any shape,
        run by md_add_noise_f16 (fp32 arithmetic, fp16 operands and result, returned in original_samples' dtype).  `timesteps`: one timestep,
        or one per entry of original_samples' first dimension.  t = 999 (abar = 0) returns the noise exactly."""
        from . import ops
        if not original_samples.is_cuda or not noise.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.add_noise: tensors must live on the GPU (no CPU path)")
        if noise.shape != original_samples.shape:
            raise ValueError(f"add_noise: noise {tuple(noise.shape)} and original_samples {tuple(original_samples.shape)} differ in shape")
        ts = [int(t) for t in torch.as_tensor(timesteps).reshape(-1).tolist()]
        if len(ts) != 1 and (original_samples.dim() == 0 or len(ts) != original_samples.shape[0]):
            raise ValueError(f"add_noise: {len(ts)} timesteps for original_samples of shape {tuple(original_samples.shape)}")
        out = noise.detach().to(torch.float16).contiguous().clone()
        x0 = original_samples.detach().to(device=out.device, dtype=torch.float16).contiguous()
        if len(ts) == 1:
            ops.add_noise(out, x0, *self.noise_coefficients(ts[0]))
        else:
            for k, t in enumerate(ts):
                ops.add_noise(out[k], x0[k], *self.noise_coefficients(t))
        return out.to(original_samples.dtype)


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class DDIMScheduler(_StrengthMixin):
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, clip_sample: bool = True, set_alpha_to_one: bool = True,
                 steps_offset: int = 0, prediction_type: str = "epsilon", thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, clip_sample_range: float = 1.0, sample_max_value: float = 1.0,
                 timestep_spacing: str = "leading", rescale_betas_zero_snr: bool = False):
        if beta_schedule != "linear" or trained_betas is not None:
            raise NotImplementedError("only beta_schedule='linear' (MikuDance config) is implemented")
        if prediction_type != "v_prediction" or timestep_spacing != "trailing" or clip_sample or thresholding:
            raise NotImplementedError("only v_prediction / trailing / clip_sample=False (MikuDance config) is implemented")
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                           steps_offset=steps_offset, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                           rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.betas = betas = _linear_betas(beta_start, beta_end, num_train_timesteps, rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_train_timesteps = num_train_timesteps
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps / num_inference_steps
        ts = np.round(np.arange(self.num_train_timesteps, 0, -ratio)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts)           # kept on the host: the loop reads them as Python ints

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step_coefficients(self, timestep):
        """(alpha_prod_t, alpha_prod_t_prev) as Python floats; prev_t = t - 1000 // N (integer division, literally)."""
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict: bool = True):
        """API-compatible step on GPU tensors of any shape (the fused pipeline calls md_cfg_ddim_step directly with
        window averaging and guidance folded in; this entry runs the same kernel without them)."""
        from . import ops
        if not sample.is_cuda or sample.numel() % 4:
            raise RuntimeError("DDIMScheduler.step: tensors must live on the GPU (no CPU path)")
        a_t, a_prev = self.step_coefficients(timestep)
        n = sample.numel() // 4
        lat = sample.detach().to(torch.float16).reshape(1, n, 4).contiguous().clone()
        v = model_output.detach().to(torch.float32).reshape(1, 1, n, 4).contiguous()
        one = torch.ones((1,), device=sample.device, dtype=torch.float32)
        z = None
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                                 " `variance_noise` stays `None`.")
            if variance_noise is None:
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
            z = variance_noise.detach().to(device=sample.device, dtype=torch.float16).reshape(1, n, 4).contiguous()
        ops.cfg_ddim_step(lat, v, one, 1, n, 1.0, a_t, a_prev, halves=1, eta=float(eta), variance_noise=z)
        prev = lat.reshape(sample.shape).to(sample.dtype)
        if not return_dict:
            return (prev,)
        return DDIMSchedulerOutput(prev_sample=prev)


@dataclass
class DPMSolverMultistepSchedulerOutput:
    prev_sample: torch.Tensor


class DPMSolverMultistepScheduler(_StrengthMixin):
    """DPM-Solver++ multistep sampling on MikuDance's zero-terminal-SNR schedule (diffusers keyword names; the built subset is
    solver_order 1 / 2, algorithm_type dpmsolver++ / sde-dpmsolver++, solver_type midpoint / heun, v-prediction, trailing spacing,
    linear betas, final_sigmas_type "zero").

    With alpha_i = sqrt(abar(t_i)), sigma_i = sqrt(1 - abar(t_i)), step i goes from s = t_i to t = t_{i+1} (the list's NEXT entry; the
    last step to the clean sample, alpha = 1, sigma = 0) and reduces to
        m0 = alpha_s x - sigma_s v,   x' = c_x x + c_m0 m0 + c_m1 m1 + c_z z     (m1 = the previous step's m0, z ~ N(0, 1))
    The coefficients use e^-h = (alpha_s sigma_t) / (sigma_s alpha_t) in float64 -- exactly 0 at the first step (alpha_s = 0) and at the
    last (sigma_t = 0) -- so lambda = log(alpha / sigma) is never formed where it is infinite.  Step 0 and the last step are order 1;
    rho = h / h_0 is 0 when the previous point is the lambda = -inf endpoint (step 1), its order-1 limit.  After set_begin_index(b) step b
    is order 1 too (sampling starts there)."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02, beta_schedule: str = "linear",
                 trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon", thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, euler_at_final: bool = False, use_karras_sigmas: bool = False,
                 use_lu_lambdas: bool = False, final_sigmas_type: str = "zero", lambda_min_clipped: float = -float("inf"),
                 variance_type=None, timestep_spacing: str = "linspace", steps_offset: int = 0, rescale_betas_zero_snr: bool = False,
                 clip_sample: bool = False, set_alpha_to_one: bool = True):
        # clip_sample / set_alpha_to_one: DDIM keys of the MikuDance config (selftest.SCHED_KWARGS), accepted at their MikuDance values
        if beta_schedule != "linear" or trained_betas is not None:
            raise NotImplementedError("only beta_schedule='linear' (MikuDance config) is implemented")
        if prediction_type != "v_prediction" or timestep_spacing != "trailing" or thresholding or clip_sample:
            raise NotImplementedError("only v_prediction / trailing / no thresholding or clipping (MikuDance config) is implemented")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order}: only orders 1 and 2 are implemented")
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: only 'dpmsolver++' and 'sde-dpmsolver++' are implemented")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_type={solver_type!r}: only 'midpoint' and 'heun' are implemented")
        if use_karras_sigmas or use_lu_lambdas:
            raise NotImplementedError("Karras / Lu lambda spacing is not implemented: timesteps follow the trailing DDIM list")
        if final_sigmas_type != "zero" or not set_alpha_to_one:
            raise NotImplementedError("only final_sigmas_type='zero' (the last step lands on the clean sample) is implemented")
        if lambda_min_clipped != -float("inf") or variance_type is not None:
            raise NotImplementedError("lambda_min_clipped / variance_type are not implemented")
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                           solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
                           dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
                           algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                           euler_at_final=euler_at_final, use_karras_sigmas=use_karras_sigmas, use_lu_lambdas=use_lu_lambdas,
                           final_sigmas_type=final_sigmas_type, lambda_min_clipped=lambda_min_clipped, variance_type=variance_type,
                           timestep_spacing=timestep_spacing, steps_offset=steps_offset, rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.betas = _linear_betas(beta_start, beta_end, num_train_timesteps, rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.init_noise_sigma = 1.0
        self.num_train_timesteps = num_train_timesteps
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._coeffs = []
        self._begin_index = 0
        self._reset_state()

    @classmethod
    def from_config(cls, config, **kwargs):
        """diffusers' from_config: keys this class does not take (e.g. a DDIMScheduler config's) are ignored."""
        known = set(inspect.signature(cls.__init__).parameters) - {"self"}
        kw = {k: v for k, v in dict(config, **kwargs).items() if k in known}
        return cls(**kw)

    @property
    def is_sde(self):
        return self.config["algorithm_type"] == "sde-dpmsolver++"

    def _reset_state(self):
        self._history = None          # fp32 data prediction of the last step taken by step()
        self._last_index = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        """The trailing list of DDIMScheduler; resets all multistep state."""
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps / num_inference_steps
        ts = np.round(np.arange(self.num_train_timesteps, 0, -ratio)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts)
        self._begin_index = 0
        self._coeffs = self._coefficient_table([int(t) for t in ts])
        self._reset_state()

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        """diffusers' name: sampling starts at step `begin_index` of the current schedule (video-to-video, get_timesteps).  That step is
        first order -- there is no history before it -- and every other row, the final-step rule included (it stays keyed on the full
        schedule), is the full table's.  multistep_coefficients keeps absolute indices; set_timesteps resets the index to 0."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        begin_index = int(begin_index)
        if not 0 <= begin_index < len(self.timesteps):
            raise ValueError(f"begin_index {begin_index} is outside the schedule of {len(self.timesteps)} steps")
        self._begin_index = begin_index
        self._coeffs = self._coefficient_table([int(t) for t in self.timesteps], begin_index)
        self._reset_state()

    def _coefficient_table(self, ts, begin=0):
        n = len(ts)
        abar = [float(self.alphas_cumprod[t]) for t in ts] + [1.0]           # final_sigmas_type "zero": alpha = 1, sigma = 0
        al = [math.sqrt(a) for a in abar]
        sg = [math.sqrt(1.0 - a) for a in abar]
        sde, heun = self.is_sde, self.config["solver_type"] == "heun"
        out, prev_emh = [], None
        for i in range(n):
            a_s, s_s, a_t, s_t = al[i], sg[i], al[i + 1], sg[i + 1]
            emh = (a_s * s_t) / (s_s * a_t)                                    # e^-h; 0 at both ends
            second = self.config["solver_order"] == 2 and 0 < i < n - 1 and i != begin          # begin: no history yet
            rho = math.log(emh) / math.log(prev_emh) if second and prev_emh > 0.0 else 0.0    # h / h_0; 0 after the lambda = -inf point
            if sde:
                c_x = s_t / s_s * emh
                g = 1.0 - emh * emh                                            # 1 - e^-2h
                k = a_t * (1.0 - g / (-2.0 * math.log(emh))) if heun and rho else 0.0
                c_z = s_t * math.sqrt(g)
            else:
                c_x = s_t / s_s
                g = 1.0 - emh
                k = a_t * (1.0 + math.expm1(math.log(emh)) / -math.log(emh)) if heun and rho else 0.0
                c_z = 0.0
            if heun:
                c_m0, c_m1 = a_t * g + k * rho, -k * rho
            else:
                c_m0, c_m1 = a_t * g * (1.0 + 0.5 * rho), -a_t * g * 0.5 * rho
            out.append((a_s, s_s, c_x, c_m0, c_m1 if rho else 0.0, c_z))
            prev_emh = emh
        return out

    def multistep_coefficients(self, step_index: int):
        """(alpha_s, sigma_s, c_x, c_m0, c_m1, c_z) of step `step_index` as Python floats (see the class docstring)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return self._coeffs[step_index]

    def index_for_timestep(self, timestep):
        t = int(timestep)
        hits = (self.timesteps == t).nonzero().flatten().tolist()
        if not hits:
            raise ValueError(f"timestep {t} is not in the current schedule ({self.num_inference_steps} steps)")
        return hits[0]

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = True):
        """API-compatible step on GPU tensors of any shape: md_cfg_multistep_step without window averaging and guidance (one clip-half,
        counter 1, guidance 1).  The step index comes from `timestep`; the scheduler keeps the fp32 data-prediction history, so a
        second-order step needs the previous step of the same schedule to have gone through this method."""
        from . import ops
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not sample.is_cuda or sample.numel() % 4:
            raise RuntimeError("DPMSolverMultistepScheduler.step: tensors must live on the GPU (no CPU path)")
        i = self.index_for_timestep(timestep)
        co = self.multistep_coefficients(i)
        n = sample.numel() // 4
        if co[4] != 0.0 and (self._history is None or self._last_index != i - 1 or self._history.numel() != 4 * n):
            raise RuntimeError(f"DPMSolverMultistepScheduler.step: step {i} is second order and needs step {i - 1} of the same schedule "
                               "(and sample shape) to have been taken first")
        if self._history is None or self._history.numel() != 4 * n or self._history.device != sample.device:
            self._history = torch.empty((1, n, 4), device=sample.device, dtype=torch.float32)
        lat = sample.detach().to(torch.float16).reshape(1, n, 4).contiguous().clone()
        v = model_output.detach().to(torch.float32).reshape(1, 1, n, 4).contiguous()
        one = torch.ones((1,), device=sample.device, dtype=torch.float32)
        z = None
        if self.is_sde:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                                 " `variance_noise` stays `None`.")
            if variance_noise is None:                                        # drawn every step, the last one included
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
            z = variance_noise.detach().to(device=sample.device, dtype=torch.float16).reshape(1, n, 4).contiguous()
        ops.cfg_multistep_step(lat, v, one, self._history, 1, n, 1.0, *co, halves=1, variance_noise=z)
        self._last_index = i
        prev = lat.reshape(sample.shape).to(sample.dtype)
        if not return_dict:
            return (prev,)
        return DPMSolverMultistepSchedulerOutput(prev_sample=prev)


@dataclass
class UniPCMultistepSchedulerOutput:
    prev_sample: torch.Tensor


def _solve(R, b):
    """R rho = b for the <= 3 x 3 systems of UniPC, float64 Gaussian elimination with partial pivoting on Python floats."""
    n = len(b)
    A = [list(R[j]) + [b[j]] for j in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda j: abs(A[j][c]))
        A[c], A[piv] = A[piv], A[c]
        for j in range(c + 1, n):
            f = A[j][c] / A[c][c]
            for k in range(c, n + 1):
                A[j][k] -= f * A[c][k]
    x = [0.0] * n
    for j in range(n - 1, -1, -1):
        x[j] = (A[j][n] - sum(A[j][k] * x[k] for k in range(j + 1, n))) / A[j][j]
    return x


class UniPCMultistepScheduler(_StrengthMixin):
    """UniPC sampling on MikuDance's schedule (diffusers keyword names; the built subset is solver_order 1 / 2 / 3, solver_type bh1 / bh2,
    predict_x0, lower_order_final, disable_corrector, v-prediction, trailing spacing, linear betas, final_sigmas_type "zero").

    With alpha_i = sqrt(abar(t_i)), sigma_i = sqrt(1 - abar(t_i)) and lambda = log(alpha / sigma), the call of step i gets the sample x the UNet
    saw at t_i (the previous step's prediction) and its v, and does, in one pass,
        m_t = alpha_i x - sigma_i v                                            the data prediction at t_i
        x^c = cc_x x_last + cc_m m_t + cc_0 H0 + cc_1 H1 + cc_2 H2             UniC-p from t_{i-1} to t_i (corrector off: x^c = x)
        x'  = pc_x x^c + pc_m m_t + pc_0 H0 + pc_1 H1                          UniP-p from t_i to t_{i+1} (the last step: to alpha = 1, sigma = 0)
        x_last <- x^c;  H0 <- m_t, H1 <- H0, H2 <- H1                          H_k: the data prediction k + 1 steps back, fp32
    For a step from s to t: h = lambda_t - lambda_s, phi_1 = expm1(-h), B = -h (bh1) or expm1(-h) (bh2), r_k = (lambda_{s-k} - lambda_s) / h,
    D_k = (m_k - m_0) / r_k, and
        UniP-p  x_t = (sigma_t / sigma_s) x_s - alpha_t phi_1 m_0 - alpha_t B sum_{k<p} rho_k D_k
        UniC-p  x_t = (sigma_t / sigma_s) x_s - alpha_t phi_1 m_0 - alpha_t B (sum_{k<p} rho_k D_k + rho_p (m_t - m_0))
    rho = [1/2] for UniP-2 and UniC-1; otherwise it solves R rho = b, rows R_j = r^(j-1) (the corrector's r_p = 1), b_j = phi_{j+1} j! / B with
    phi_{k+1} = phi_k / (-h) - 1 / k!.  The systems are solved here in float64; the kernel only sees the weights.  lambda differences are taken
    as log((alpha_a sigma_b) / (sigma_a alpha_b)), never as a difference of two logarithms.

    The rules of the table (unipc_coefficients), with b = begin_index (0 unless set_begin_index was called):
      * predictor order of step i = min(solver_order, steps left n - i, 1 + usable history), the usable history being the run of steps
        i - 1, i - 2, ... >= b whose lambda is finite: t = 999 of a zero-terminal-SNR table (lambda = -inf) is no D_k, as DPM-Solver++'s
        rho = 0 there;
      * the corrector of step i has the order the predictor of step i - 1 had; none at step 0, none at step b (nothing before it), none at a
        step listed in disable_corrector, none behind the last step: the result is the last predictor's output, which is m_t (sigma = 0);
      * a corrector out of the lambda = -inf point has h = inf: bh2's B = -1 there and the update is finite (order 1:
        sigma_t x_s + alpha_t (m_0 + m_t) / 2); bh1's B = -h is unbounded, so under bh1 that one step has no corrector;
      * every entry of every row is finite, and a weight that is not used is exactly 0.
    The kernel reads a plane only where one of its two weights is non-zero, and moves down (H_k -> H_{k+1}) only the planes it read.  That is
    enough: H_k is needed as H_{k+1} at step i + 1 only by a corrector of order >= k + 2 or a predictor of order >= k + 3 there, and either
    means a predictor of order >= k + 2 at step i (the corrector repeats its order; the predictor's order grows by at most one a step), which
    gave H_k a non-zero weight.  So the first step runs on an uninitialised state and nothing has to be cleared between FreeInit passes or at
    a video-to-video start (tests/test_unipc_cpu.py follows every plane through every table)."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02, beta_schedule: str = "linear",
                 trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon", thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, predict_x0: bool = True, solver_type: str = "bh2",
                 lower_order_final: bool = True, disable_corrector=(), solver_p=None, use_karras_sigmas: bool = False,
                 timestep_spacing: str = "linspace", steps_offset: int = 0, final_sigmas_type: str = "zero", rescale_betas_zero_snr: bool = False,
                 clip_sample: bool = False, set_alpha_to_one: bool = True):
        # clip_sample / set_alpha_to_one: DDIM keys of the MikuDance config (selftest.SCHED_KWARGS), accepted at their MikuDance values
        if beta_schedule != "linear" or trained_betas is not None:
            raise NotImplementedError("only beta_schedule='linear' (MikuDance config) is implemented")
        if prediction_type != "v_prediction" or timestep_spacing != "trailing" or thresholding or clip_sample:
            raise NotImplementedError("only v_prediction / trailing / no thresholding or clipping (MikuDance config) is implemented")
        if solver_order not in (1, 2, 3):
            raise NotImplementedError(f"solver_order={solver_order}: only orders 1, 2 and 3 are implemented")
        if solver_type not in ("bh1", "bh2"):
            raise NotImplementedError(f"solver_type={solver_type!r}: only 'bh1' and 'bh2' are implemented")
        if not predict_x0 or not lower_order_final or solver_p is not None:
            raise NotImplementedError("only predict_x0=True, lower_order_final=True and solver_p=None are implemented")
        if use_karras_sigmas:
            raise NotImplementedError("Karras spacing is not implemented: timesteps follow the trailing DDIM list")
        if final_sigmas_type != "zero" or not set_alpha_to_one:
            raise NotImplementedError("only final_sigmas_type='zero' (the last step lands on the clean sample) is implemented")
        disable_corrector = [int(i) for i in disable_corrector]
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                           solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
                           dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value, predict_x0=predict_x0,
                           solver_type=solver_type, lower_order_final=lower_order_final, disable_corrector=disable_corrector, solver_p=solver_p,
                           use_karras_sigmas=use_karras_sigmas, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                           final_sigmas_type=final_sigmas_type, rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.betas = _linear_betas(beta_start, beta_end, num_train_timesteps, rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.init_noise_sigma = 1.0
        self.num_train_timesteps = num_train_timesteps
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._coeffs = []
        self._begin_index = 0
        self._reset_state()

    @classmethod
    def from_config(cls, config, **kwargs):
        """diffusers' from_config: keys this class does not take (e.g. a DDIMScheduler config's) are ignored."""
        known = set(inspect.signature(cls.__init__).parameters) - {"self"}
        kw = {k: v for k, v in dict(config, **kwargs).items() if k in known}
        return cls(**kw)

    def _reset_state(self):
        self._state = None           # fp32 (4, n, 4): x_last, H0, H1, H2 of the steps taken by step()
        self._last_index = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        """The trailing list of DDIMScheduler; resets the begin index and all multistep state."""
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps / num_inference_steps
        ts = np.round(np.arange(self.num_train_timesteps, 0, -ratio)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts)
        self._begin_index = 0
        self._coeffs = self._coefficient_table([int(t) for t in ts])
        self._reset_state()

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        """diffusers' name: sampling starts at step `begin_index` of the current schedule (video-to-video, get_timesteps).  That step has no
        corrector and a first-order predictor, and the orders ramp up from it; unipc_coefficients keeps absolute indices (rows in front of
        begin_index are the full table's); set_timesteps resets the index to 0."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        begin_index = int(begin_index)
        if not 0 <= begin_index < len(self.timesteps):
            raise ValueError(f"begin_index {begin_index} is outside the schedule of {len(self.timesteps)} steps")
        self._begin_index = begin_index
        self._coeffs = self._coefficient_table([int(t) for t in self.timesteps], begin_index)
        self._reset_state()

    def _coefficient_table(self, ts, begin=0):
        n = len(ts)
        abar = [float(self.alphas_cumprod[t]) for t in ts] + [1.0]           # final_sigmas_type "zero": alpha = 1, sigma = 0
        al = [math.sqrt(a) for a in abar]
        sg = [math.sqrt(1.0 - a) for a in abar]
        bh1, K, off = self.config["solver_type"] == "bh1", self.config["solver_order"], set(self.config["disable_corrector"])

        def dlam(a, b):
            """lambda_a - lambda_b; -inf / +inf where one of them is an end of a zero-terminal-SNR schedule."""
            num, den = al[a] * sg[b], sg[a] * al[b]
            return -math.inf if num == 0.0 else math.inf if den == 0.0 else math.log(num / den)

        def update(s, t, p, corrector):
            """The weights of UniP-p / UniC-p from point s to point t on (x_s, m_t or None, m_0, m_1, m_2), or None where they are not finite."""
            h = dlam(t, s)
            hh = -h
            phi1 = math.expm1(hh) if math.isfinite(h) else -1.0
            B = hh if bh1 else phi1
            rks = [dlam(s - k, s) / h for k in range(1, p)] + ([1.0] if corrector else [])
            if not rks:
                rho = []
            elif not math.isfinite(B):
                return None
            elif len(rks) == 1 and (corrector or p == 2):
                rho = [0.5]
            else:
                b, phik, fact = [], phi1 / hh - 1.0, 1.0
                for j in range(1, len(rks) + 1):
                    b.append(phik * fact / B)
                    fact *= j + 1
                    phik = phik / hh - 1.0 / fact
                rho = _solve([[r ** j for r in rks] for j in range(len(rks))], b)
            w = [sg[t] / sg[s], 0.0, -al[t] * phi1, 0.0, 0.0]
            for k in range(1, p):
                w[2 + k] = -al[t] * B * rho[k - 1] / rks[k - 1]
                w[2] -= w[2 + k]
            if corrector:
                w[1] = -al[t] * B * rho[-1]
                w[2] -= w[1]
            return [v if v else 0.0 for v in w]                                # no -0.0

        usable = [al[j] > 0.0 and sg[j] > 0.0 for j in range(n)]
        out, orders = [], []
        for i in range(n):
            lo = begin if i >= begin else 0
            hist = 0
            while i - 1 - hist >= lo and usable[i - 1 - hist]:
                hist += 1
            p = min(K, n - i, hist + 1)
            orders.append(p)
            cw = update(i - 1, i, orders[i - 1], True) if i > lo and i not in off else None
            pw = update(i, i + 1, p, False)
            row = (al[i], sg[i]) + tuple(cw or [0.0] * 5) + (pw[0], pw[2], pw[3], pw[4]) + (cw is not None,)
            assert all(math.isfinite(v) for v in row), (i, row)
            out.append(row)
        return out

    def unipc_coefficients(self, step_index: int):
        """The row of step `step_index` (see the class docstring): (alpha_s, sigma_s, cc_x, cc_m, cc_0, cc_1, cc_2, pc_x, pc_m, pc_0, pc_1) as
        Python floats and, last, whether the corrector runs (bool; False: the five cc are 0 and x^c = x)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return self._coeffs[step_index]

    def index_for_timestep(self, timestep):
        t = int(timestep)
        hits = (self.timesteps == t).nonzero().flatten().tolist()
        if not hits:
            raise ValueError(f"timestep {t} is not in the current schedule ({self.num_inference_steps} steps)")
        return hits[0]

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        """API-compatible step on GPU tensors of any shape: md_cfg_unipc_step without window averaging and guidance (one clip-half,
        counter 1, guidance 1).  The step index comes from `timestep`; the scheduler keeps the fp32 state (x_last and three data predictions),
        so a step whose row reads it needs the previous step of the same schedule to have gone through this method."""
        from . import ops
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not sample.is_cuda or sample.numel() % 4:
            raise RuntimeError("UniPCMultistepScheduler.step: tensors must live on the GPU (no CPU path)")
        i = self.index_for_timestep(timestep)
        row = self.unipc_coefficients(i)
        n = sample.numel() // 4
        fresh = self._state is None or self._state.numel() != 16 * n or self._state.device != sample.device
        if (row[11] or row[9] != 0.0 or row[10] != 0.0) and (fresh or self._last_index != i - 1):
            raise RuntimeError(f"UniPCMultistepScheduler.step: step {i} reads the state of step {i - 1} of the same schedule (and sample "
                               "shape), which has to be taken first")
        if fresh:
            self._state = torch.empty((4, n, 4), device=sample.device, dtype=torch.float32)
        lat = sample.detach().to(torch.float16).reshape(1, n, 4).contiguous().clone()
        v = model_output.detach().to(torch.float32).reshape(1, 1, n, 4).contiguous()
        one = torch.ones((1,), device=sample.device, dtype=torch.float32)
        ops.cfg_unipc_step(lat, v, one, self._state, 1, n, 1.0, row, halves=1)
        self._last_index = i
        prev = lat.reshape(sample.shape).to(sample.dtype)
        if not return_dict:
            return (prev,)
        return UniPCMultistepSchedulerOutput(prev_sample=prev)
