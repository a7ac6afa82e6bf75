"""CPU: DeepCache (deep_cache_interval=, deep_cache_depth=; forward_nhwc(deep_cache=)) on the emulated operator layer (tests/fake_ops.py): the host
graph of a key step and of a shallow step, the loop's schedule of key steps, every refusal.  The restatement is tests/deepcache_ref.py.

Bounds.  Replay (fill, then reuse on the SAME inputs) is bitwise the full call: the shallow layers see the same operands.  Reuse on other inputs
against the fp32 restatement: rel-L2 < 2e-2 and cosine > 0.999, the bound tests/test_host_graph_cpu.py uses for a full forward."""
import pytest
import torch
import torch.distributed as dist

import deepcache_ref as DR
import fake_ops
import mikudance_amd as M
from loop_helpers import CountingUNet, run_world, small_cpu, small_inputs, worker_setup, zero_inputs  # noqa: F401
from mikudance_amd import DeepCacheSlot, blocks
from mikudance_amd.selftest import SCHED_KWARGS, cosine, rel_l2
from mikudance_amd.synth import synth_inputs

F_, G = 2, 3.5
DEPTHS = (1, 2, 3, 4, 6)


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _inputs(seed, f=F_, h=16, w=16):
    return tuple(t.half().float() for t in synth_inputs(f, h, w, ctx_len=5, ctx_dim=64, seed=seed))


@pytest.fixture()
def banked(small_cpu, monkeypatch):
    """The small models on the emulated operators with the reference banks of seed-5 inputs in the denoising UNet's blocks."""
    ref, den, ref_sd, den_sd = small_cpu
    fake_ops.install(monkeypatch)
    lat, rl, emb = _inputs(5)
    writer, reader = DR.write_banks(ref, den, rl, emb, F_, 16, 16)
    yield den, den_sd, ref_sd, lat, rl, emb
    reader.clear()
    writer.clear()
    den.clear_context_cache()
    ref.clear_context_cache()


def _two(lat):
    return lat.repeat(2, 1, 1, 1, 1).half()


# ---- 1. the default is the plain call
def test_no_slot_is_the_plain_forward(banked):
    den, _, _, lat, _, emb = banked
    del fake_ops.CALLS[:]
    a = DR.call_nhwc(den, _two(lat), 601, emb.half(), halves_identical=True)
    calls_a = list(fake_ops.CALLS)
    del fake_ops.CALLS[:]
    b = DR.call_nhwc(den, _two(lat), 601, emb.half(), halves_identical=True, deep_cache=None)
    assert torch.equal(a, b) and calls_a == fake_ops.CALLS


def test_interval_one_is_the_same_call_log_and_the_same_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(3, 19))
    keywords = []
    real = den.forward_nhwc

    def forward_nhwc(*a, **kw):
        keywords.append(sorted(kw))
        return real(*a, **kw)

    monkeypatch.setattr(den, "forward_nhwc", forward_nhwc, raising=False)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    a = pipe.denoise(lat, rl, emb, 2, G)
    calls_a = list(fake_ops.CALLS)
    for kw in (dict(deep_cache_interval=1), dict(deep_cache_interval=1, deep_cache_depth=5)):
        del fake_ops.CALLS[:]
        b = pipe.denoise(lat, rl, emb, 2, G, **kw)
        assert torch.equal(a, b) and calls_a == fake_ops.CALLS             # the same operator calls, one for one
    assert all(k == ["halves_identical", "two_queues"] for k in keywords), keywords      # no new keyword reaches forward_nhwc
    del keywords[:]
    c = pipe.denoise(lat, rl, emb, 2, G, deep_cache_interval=2)
    assert not torch.equal(a, c)
    assert all(k == ["deep_cache", "halves_identical", "two_queues"] for k in keywords), keywords
    plan = pipe.sampling_plan(2, G, False, (3, 16, 16), guidance_rescale=0.0, strength=1.0, context_fuse="flat", free_init_iters=1,
                              free_init_filter="butterworth", free_init_order=4, free_init_spatial_stop=0.25, free_init_temporal_stop=0.25,
                              free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0, pag_scale=0.0,
                              pag_adaptive_scale=0.0, pag_applied_layers=("mid",), kv_downsample=1, kv_downsample_mode="nearest", seg_scale=0.0,
                              seg_blur_sigma=100.0, seg_applied_layers=("mid",), deep_cache_interval=1, deep_cache_depth=4)
    assert plan.deep is None


# ---- 2. replay: fill, then reuse on the same inputs, is the full call
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("d", DEPTHS)
def test_replay_is_bitwise_the_full_call(banked, d, share):
    den, _, _, lat, _, emb = banked
    x = _two(lat)
    full = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=share)
    slot = DeepCacheSlot(d)
    a = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=share, deep_cache=slot)
    n_full = len(fake_ops.CALLS)
    b = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=share, deep_cache=slot.reuse())
    assert torch.equal(a, full) and torch.equal(b, full)
    assert len(fake_ops.CALLS) - n_full < n_full / 3 * 2                  # and it ran less
    c = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=share, deep_cache=slot.reuse())      # the kept hidden state survives a reuse
    assert torch.equal(c, full)


@pytest.mark.parametrize("d", (1, 3, 4))
def test_replay_of_a_perturbed_call(banked, d):
    den, _, _, lat, _, emb = banked
    pag = den.pag_blocks(("down_blocks.0", "mid_block"))
    x = lat.half()
    full = DR.call_nhwc(den, x, 601, emb[1:].half(), pag=pag)
    slot = DeepCacheSlot(d)
    a = DR.call_nhwc(den, x, 601, emb[1:].half(), pag=pag, deep_cache=slot)
    b = DR.call_nhwc(den, x, 601, emb[1:].half(), pag=pag, deep_cache=slot.reuse())
    assert torch.equal(a, full) and torch.equal(b, full)


# ---- 3. reuse on other inputs against the fp32 restatement
@pytest.mark.parametrize("hw,d", [((16, 16), 1), ((16, 16), 3), ((16, 16), 4), ((16, 16), 6), ((12, 20), 4), ((12, 20), 7)])
def test_shallow_step_matches_the_literal_reference(small_cpu, monkeypatch, hw, d):
    """(12, 20): levels 12x20 / 6x10 / 3x5 / 2x3 -- the force_size upsampler of up_blocks.2 (6x10 from 3x5) is on the shallow side at d = 7,
    up_blocks.2's plain one at d = 4."""
    ref, den, ref_sd, den_sd = small_cpu
    fake_ops.install(monkeypatch)
    h, w = hw
    lat1, rl, emb = _inputs(5, h=h, w=w)
    lat2 = _inputs(6, h=h, w=w)[0]
    t1, t2 = 601, 401
    assert not torch.equal(lat1, lat2)
    writer, reader = DR.write_banks(ref, den, rl, emb, F_, h, w)
    try:
        slot = DeepCacheSlot(d)
        DR.call_nhwc(den, _two(lat1), t1, emb.half(), halves_identical=True, deep_cache=slot)
        got = DR.call_nhwc(den, _two(lat2), t2, emb.half(), halves_identical=True, deep_cache=slot.reuse())
        plain = DR.call_nhwc(den, _two(lat2), t2, emb.half(), halves_identical=True)
    finally:
        reader.clear(); writer.clear(); den.clear_context_cache(); ref.clear_context_cache()
    banks = DR.oracle_banks(ref_sd, rl, emb, F_, h, w)
    with torch.no_grad():
        _, hidden = DR.full(den_sd, lat1.repeat(2, 1, 1, 1, 1), torch.tensor(t1), emb, banks)
        want = DR.shallow(den_sd, lat2.repeat(2, 1, 1, 1, 1), torch.tensor(t2), emb, banks, True, d, hidden[d - 1])
        want_full, _ = DR.full(den_sd, lat2.repeat(2, 1, 1, 1, 1), torch.tensor(t2), emb, banks)
        assert torch.equal(want_full, __import__("oracle.cpu_ref", fromlist=["x"]).denoising_unet_forward(
            den_sd, lat2.repeat(2, 1, 1, 1, 1), torch.tensor(t2), emb, banks, cfg=True))         # the restated walk is the oracle's forward
    r, c = rel_l2(got, want), cosine(got, want)
    print(f"\nDEEPCACHE_HOST {h}x{w} d{d}: rel_l2 {r:.3e} cos {c:.7f}; full vs shallow reference {rel_l2(want_full, want):.3e}")
    assert r < 2e-2 and c > 0.999, (r, c)
    assert rel_l2(plain, want_full) < 2e-2
    assert rel_l2(got, plain) > 0                                          # the deep part really is the other step's


# ---- 4. what does not run
def _names(den):
    return {m: n for n, m in den.named_modules()}


def _traced(den, monkeypatch, fn):
    """Run fn() -> (result, [(layer name or None, logged call)], layers entered, context_kv blocks, bank reads, time-row reads)."""
    kinds = (blocks.ResnetBlock, blocks.SpatialTransformer, blocks.MotionModule, blocks.ConvSampler)
    names = _names(den)
    owner, entered, hooks, marks = [None], [], [], []
    for m, n in names.items():
        if isinstance(m, kinds):
            hooks.append(m.register_forward_pre_hook(lambda mod, a, n=n: (owner.__setitem__(0, n), entered.append(n), marks.append((len(fake_ops.CALLS), n)))[0]))
            hooks.append(m.register_forward_hook(lambda mod, a, o: (owner.__setitem__(0, None), marks.append((len(fake_ops.CALLS), None)))[0]))
    ctx_kv, bank_reads, temb_reads = [], [], []
    real_kv = blocks.TransformerBlock.context_kv

    def context_kv(self, cross):
        if self._kv_cache is None or self._kv_cache[0] is not cross.root:
            ctx_kv.append(names[self])
        return real_kv(self, cross)

    class Bank(list):
        def __getitem__(self, i):
            bank_reads.append(self.name)
            return list.__getitem__(self, i)

    real_temb = type(den)._temb

    def temb(self, pk, trows, r):
        temb_reads.append(names[r])
        return real_temb(self, pk, trows, r)

    monkeypatch.setattr(blocks.TransformerBlock, "context_kv", context_kv)
    monkeypatch.setattr(type(den), "_temb", temb)
    saved = {}
    for tb in den.transformer_blocks_in_order():
        saved[tb] = tb.bank
        b = Bank(tb.bank)
        b.name = names[tb]
        tb.bank = b
    start = len(fake_ops.CALLS)
    try:
        out = fn()
    finally:
        for h in hooks:
            h.remove()
        for tb, b in saved.items():
            tb.bank = b
        monkeypatch.undo()
    calls, cur, mi = [], None, 0
    for i in range(start, len(fake_ops.CALLS)):
        while mi < len(marks) and marks[mi][0] <= i:
            cur = marks[mi][1]
            mi += 1
        calls.append((cur, fake_ops.CALLS[i]))
    return out, calls, entered, ctx_kv, bank_reads, temb_reads


def _layer_of(name):
    """'down_blocks.0.attentions.1' -> ('down_blocks.0', 1); samplers -> (block, 'sampler'); mid -> ('mid_block', j)."""
    parts = name.split(".")
    if parts[0] == "mid_block":
        return ("mid_block", None)
    blk = ".".join(parts[:2])
    return (blk, "sampler") if parts[2] in ("downsamplers", "upsamplers") else (blk, int(parts[3]))


def _expected_layers(d):
    """The (block, layer) pairs a shallow step of depth d runs on the 4-level geometry, from the issue's text and nothing else."""
    down = [("down_blocks.%d" % i, j) for i in range(4) for j in ((0, 1, "sampler") if i < 3 else (0, 1))]
    up = [("up_blocks.%d" % i, j) for i in range(4) for j in (0, 1, 2)]
    run = set(down[:d - 1]) | set(up[len(up) - d:])
    for i in range(3):                                                     # an upsampler runs where it lies between two layers that run
        if ("up_blocks.%d" % i, 2) in run:
            run.add(("up_blocks.%d" % i, "sampler"))
    return run


@pytest.mark.parametrize("d", DEPTHS)
def test_a_reuse_call_runs_the_shallow_layers_only(small_cpu, d):
    ref, den, _, _ = small_cpu
    mp = pytest.MonkeyPatch()
    fake_ops.install(mp)
    try:
        lat, rl, emb = _inputs(5)
        writer, reader = DR.write_banks(ref, den, rl, emb, F_, 16, 16)
        x = _two(lat)
        slot = DeepCacheSlot(d)
        den.clear_context_cache()
        inner = pytest.MonkeyPatch()
        _, full_calls, full_entered, kv_full, _, _ = _traced(den, inner, lambda: DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot))
        assert len(kv_full) == 16                                          # a new context: every block projects it
        den.clear_context_cache()                                          # the context is NEW for the reuse call
        emb2 = (emb * 0.5).half()
        _, calls, entered, kv, bank_reads, temb_reads = _traced(den, pytest.MonkeyPatch(), lambda: DR.call_nhwc(den, x, 401, emb2, halves_identical=True,
                                                                                                              deep_cache=slot.reuse()))
        reader.clear(); writer.clear(); den.clear_context_cache(); ref.clear_context_cache()
    finally:
        mp.undo()
    want = _expected_layers(d)
    assert {_layer_of(n) for n in entered} == want, (sorted(map(str, {_layer_of(n) for n in entered})), sorted(map(str, want)))
    assert len(entered) == len(set(entered))
    # context_kv, bank reads and time rows: of layers that run only
    attn = lambda n: _layer_of(n.replace(".transformer_blocks.0", ""))
    assert {attn(n) for n in kv} <= want and len(kv) == len({l for l in want if l[1] != "sampler" and l[0] != "up_blocks.0" and l[0] != "down_blocks.3"})
    assert {attn(n) for n in bank_reads} <= want and bank_reads
    assert {_layer_of(n) for n in temb_reads} <= want and len(temb_reads) == len([l for l in want if l[1] != "sampler"])
    # the launches that do run are exactly the full call's launches for those layers (and the ones outside any layer: time rows, conv_in, the output)
    keep = [(n, c) for n, c in full_calls if n is None or _layer_of(n) in want]
    assert [c for _, c in keep] == [c for _, c in calls]
    assert [n for n, _ in keep] == [n for n, _ in calls]


# ---- 5. the loop
class _Spy:
    """Records every forward_nhwc call of a denoise(): (perturbed?, mode, serial number of the slot's store, ...) and the window of the accumulate behind it."""

    def __init__(self, den, monkeypatch):
        self.calls, self.stores = [], []                                   # (the stores are held: a serial number per living object)
        real = den.forward_nhwc

        def sid(store):
            if not any(store is s for s in self.stores):
                self.stores.append(store)
            return [store is s for s in self.stores].index(True)

        def forward_nhwc(x, nb, f, t, cross, **kw):
            dc = kw.get("deep_cache")
            self.calls.append(dict(pert="pag" in kw or "seg" in kw, mode=None if dc is None else dc.mode, store=None if dc is None else sid(dc.store),
                                   depth=None if dc is None else dc.depth, t=float(t[0]), shift=kw.get("tile_shift")))
            return real(x, nb, f, t, cross, **kw)

        monkeypatch.setattr(den, "forward_nhwc", forward_nhwc, raising=False)
        from mikudance_amd import ops
        acc = ops.window_accumulate

        def window_accumulate(pred, planes, count, window, *a, **k):
            self.calls[-1]["window"] = window.tolist()
            return acc(pred, planes, count, window, *a, **k)

        monkeypatch.setattr(ops, "window_accumulate", window_accumulate)

    def by_step(self):
        """[[call, ...] per executed step], a step = a run of calls at one t (passes concatenated)."""
        out = []
        for c in self.calls:
            if not out or out[-1][0]["t"] != c["t"] or (not c["pert"] and any(o["window"] == c.get("window") and not o["pert"] for o in out[-1])):
                out.append([])
            out[-1].append(c)
        return out


def _modes(spy, pert=False):
    return [sorted({c["mode"] for c in step if c["pert"] == pert}) for step in spy.by_step()]


@pytest.mark.parametrize("n", [2, 3])
def test_key_steps_fall_at_multiples_of_the_interval(monkeypatch, small_cpu, n):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 31))
    spy = _Spy(den, monkeypatch)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    out = pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=n, deep_cache_depth=3)
    assert torch.isfinite(out).all()
    assert _modes(spy) == [["fill"] if k % n == 0 else ["reuse"] for k in range(5)]
    assert {c["depth"] for c in spy.calls} == {3} and len({c["store"] for c in spy.calls}) == 1


def test_count_restarts_per_free_init_pass_and_at_the_first_kept_step(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 32))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    spy = _Spy(den, monkeypatch)
    pipe.denoise(lat, rl, emb, 3, G, deep_cache_interval=2, free_init_iters=2, generator=torch.Generator().manual_seed(1))
    assert _modes(spy) == [["fill"], ["reuse"], ["fill"]] * 2
    stores = [c["store"] for c in spy.calls]
    assert stores[0] == stores[1] == stores[2] and stores[3] == stores[4] == stores[5] and stores[0] != stores[3]      # an empty cache per pass
    # strength 0.5 of 6 steps keeps the last 3: k = 0 is the first KEPT step, whatever its index in the schedule
    spy = _Spy(den, monkeypatch)
    pipe.denoise(lat, rl, emb, 6, G, deep_cache_interval=2, init_latents=lat * 0.5, strength=0.5)
    assert _modes(spy) == [["fill"], ["reuse"], ["fill"]]
    spy = _Spy(den, monkeypatch)
    pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=2, init_latents=lat * 0.5, strength=0.8)      # 4 kept steps, t_start = 1 (odd)
    assert _modes(spy) == [["fill"], ["reuse"], ["fill"], ["reuse"]]


def test_long_clip_windows_of_a_shallow_step_are_its_key_steps(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(6, 33))
    spy = _Spy(den, monkeypatch)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=2, context_frames=4, context_stride=1, context_overlap=2)
    steps = spy.by_step()
    assert len(steps) == 4 and len(steps[0]) > 1
    for k in (0, 2):
        key, sh = steps[k], steps[k + 1]
        assert [c["mode"] for c in key] == ["fill"] * len(key) and [c["mode"] for c in sh] == ["reuse"] * len(key)
        assert [(c["window"], c["store"]) for c in key] == [(c["window"], c["store"]) for c in sh]
    assert len({c["store"] for c in steps[0]}) == len(steps[0])            # one slot per window
    assert not den._cross_cache


def test_adaptive_pag_fills_and_reuses_consistently(monkeypatch, small_cpu):
    """4 trailing steps: t = 999, 749, 499, 249; scale 3 - 0.008 (1000 - t) = 2.99, 0.99, 0, 0: the perturbed plane stops after step 1."""
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 34))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    kw = dict(pag_scale=3.0, pag_adaptive_scale=0.008, pag_applied_layers=("down_blocks.0",))
    for n, main, pert in ((2, ["fill", "reuse", "fill", "reuse"], [["fill"], ["reuse"], [], []]),
                          (3, ["fill", "reuse", "reuse", "fill"], [["fill"], ["reuse"], [], []])):
        spy = _Spy(den, monkeypatch)
        out = pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=n, **kw)
        assert torch.isfinite(out).all()
        assert _modes(spy) == [[m] for m in main] and _modes(spy, pert=True) == pert
        main_store = {c["store"] for c in spy.calls if not c["pert"]}
        pert_store = {c["store"] for c in spy.calls if c["pert"]}
        assert len(main_store) == 1 and len(pert_store) == 1 and main_store != pert_store      # one slot per plane
    plain = pipe.denoise(lat, rl, emb, 4, G, **kw)
    assert not torch.equal(plain, out)


def test_tile_shift_stays_a_function_of_the_step(monkeypatch, small_cpu):
    import tile_ref
    fake_ops.install(monkeypatch)
    tile_ref.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 35))
    spy = _Spy(den, monkeypatch)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=2, tile_attention=2, kv_downsample=2)
    assert [c["shift"] for c in spy.calls] == [0, 1, 2, 3] and [c["mode"] for c in spy.calls] == ["fill", "reuse", "fill", "reuse"]


def test_nothing_outlives_denoise(monkeypatch, small_cpu):
    import gc
    import weakref
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 36))
    kept = []
    real = den.forward_nhwc

    def forward_nhwc(*a, **kw):
        out = real(*a, **kw)
        kept.extend(weakref.ref(b) for b in kw["deep_cache"].store["bufs"].values())
        return out

    monkeypatch.setattr(den, "forward_nhwc", forward_nhwc, raising=False)
    M.MikuDanceVideoPipeline(None, None, ref, den, _ddim()).denoise(lat, rl, emb, 2, G, deep_cache_interval=2)
    gc.collect()
    assert kept and all(r() is None for r in kept)


WP = dict(context_frames=8, context_stride=1, context_overlap=2)           # 16 frames: 3 windows, the last one wraps


def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    kw = dict(WP, deep_cache_interval=2)
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat, rl, emb, 2, G, window_parallel=dp.WindowParallel(), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        one = pipe.denoise(lat, rl, emb, 2, G, **kw)
        plain = pipe.denoise(lat, rl, emb, 2, G, **WP)
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), cached=not torch.equal(out, plain)))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert all(res.values()), res


# ---- 6. refusals
def test_forward_refusals(banked):
    den, _, _, lat, _, emb = banked
    x = _two(lat)
    for d in (0, 12, 13, -1):
        with pytest.raises(ValueError, match=f"deep_cache_depth.*got {d}"):
            DR.call_nhwc(den, x, 601, emb.half(), deep_cache=DeepCacheSlot(d) if d >= 1 else type("S", (), dict(depth=d, mode="fill", store={}))())
    for bad in (0, -3, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="deep_cache_depth must be an integer >= 1"):
            DeepCacheSlot(bad)
    with pytest.raises(ValueError, match="mode must be one of"):
        DeepCacheSlot(3, "keep")
    n = len(fake_ops.CALLS)
    with pytest.raises(ValueError, match="reuse with an empty slot"):
        DR.call_nhwc(den, x, 601, emb.half(), deep_cache=DeepCacheSlot(3, "reuse"))
    slot = DeepCacheSlot(3)
    DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot)
    n = len(fake_ops.CALLS)
    with pytest.raises(ValueError, match=r"halves_identical\) = \(2, 2, False, False\), the fill call had \(2, 2, False, True\)"):
        DR.call_nhwc(den, x, 601, emb.half(), deep_cache=slot.reuse())
    with pytest.raises(ValueError, match=r"= \(2, 2, True, True\), the fill call had"):
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, two_queues=True, deep_cache=slot.reuse())
    with pytest.raises(ValueError, match=r"= \(1, 2, False, False\), the fill call had"):
        DR.call_nhwc(den, lat.half(), 601, emb[1:].half(), deep_cache=slot.reuse())
    with pytest.raises(ValueError, match=r"= \(2, 1, False, True\), the fill call had"):
        DR.call_nhwc(den, x[:, :, :1], 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())
    # a buffer that does not fit: another latent size, another depth's buffer, another dtype
    with pytest.raises(ValueError, match=r"the kept buffer \(4, 16, 16, 192\) torch.float16 on cpu does not fit this call, which needs \(4, 8, 8, 192\)"):
        DR.call_nhwc(den, x[..., :8, :8], 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())
    with pytest.raises(ValueError, match="does not fit this call"):
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=DeepCacheSlot(4, "reuse", slot.store))
    good = slot.store["bufs"][0]
    slot.store["bufs"][0] = good.float()
    with pytest.raises(ValueError, match="torch.float32 on cpu does not fit"):
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())
    slot.store["bufs"][0] = good
    assert len([c for c in fake_ops.CALLS[n:] if c[0] in ("gemm", "conv")]) == 0      # every refusal came before the first launch
    DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())
    slot.drop()
    with pytest.raises(ValueError, match="reuse with an empty slot"):
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())


@pytest.mark.parametrize("kw,msg", [(dict(deep_cache_interval=0), "deep_cache_interval must be an integer >= 1, got 0"),
                                    (dict(deep_cache_interval=-2), "deep_cache_interval must be an integer >= 1, got -2"),
                                    (dict(deep_cache_interval=2.0), "deep_cache_interval must be an integer >= 1, got 2.0"),
                                    (dict(deep_cache_interval=True), "deep_cache_interval must be an integer >= 1, got True"),
                                    (dict(deep_cache_interval="2"), "deep_cache_interval must be an integer >= 1, got '2'"),
                                    (dict(deep_cache_depth=0), "deep_cache_depth must be an integer >= 1, got 0"),
                                    (dict(deep_cache_interval=2, deep_cache_depth=1.5), "deep_cache_depth must be an integer >= 1, got 1.5"),
                                    (dict(deep_cache_depth=None), "deep_cache_depth must be an integer >= 1, got None")])
def test_loop_refusals_come_before_any_unet(kw, msg):
    ref, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 2, G, **kw)
    assert ref.calls == den.calls == 0


def test_depth_out_of_range_is_refused_against_the_unet(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 37))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    for d in (12, 40):
        with pytest.raises(ValueError, match=f"deep_cache_depth must be in 1..11 for this UNet \\(12 skip tensors\\), got {d}"):
            pipe.denoise(lat, rl, emb, 2, G, deep_cache_interval=2, deep_cache_depth=d)
    assert not [c for c in fake_ops.CALLS if c[0] == "gemm"]               # nothing ran
    pipe.denoise(lat, rl, emb, 2, G, deep_cache_interval=2, deep_cache_depth=11)


def test_script_flags():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.deep_cache_interval, a.deep_cache_depth) == (1, 3)
    a = IV.parse_args(["--deep_cache_interval", "3", "--deep_cache_depth", "2"])
    assert (a.deep_cache_interval, a.deep_cache_depth) == (3, 2)
    with pytest.raises(SystemExit):
        IV.parse_args(["--deep_cache_interval", "two"])
    assert "deep_cache_interval=--deep_cache_interval" in IV.__doc__
