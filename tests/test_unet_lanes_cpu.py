"""CPU: the two-lane schedule of UNet3DConditionModel.forward_nhwc(two_queues=True) -- one lane per clip-half -- on the emulated operator layer
(tests/fake_ops.py).  unet_3d_mix._side_streams is the one seam: patched to a pair of None the lanes run inline, with no streams or events, through
the same schedule that forks them onto two kernel queues on the GPU.  And two corners of the shared walk: the hand-over of a key step whose
shared first resnet pushes a skip of its own, and the dead tail of the reference UNet.

Every comparison is between runs whose operators see the same shapes: the criterion is torch.equal, there is no tolerance."""
import math

import pytest
import torch

import deepcache_adaptive_ref as AR
import deepcache_ref as DR
import fake_ops
import mikudance_amd as M
from loop_helpers import small_cpu  # noqa: F401
from mikudance_amd import DeepCacheSlot, ops, unet_3d_mix
from test_deep_cache_cpu import DEPTHS, _inputs, _two

F_, T = 3, 601


@pytest.fixture()
def two_lanes(small_cpu, monkeypatch):
    """test_deep_cache_cpu's `banked` setting at 3 frames, with a pair of None for the lane streams: (den, both halves' latents, embeds)."""
    ref, den, _, _ = small_cpu
    fake_ops.install(monkeypatch)
    AR.install(monkeypatch)
    monkeypatch.setattr(unet_3d_mix, "_side_streams", lambda x: (None, None))
    den.packed().pop("_two_queue_shapes", None)
    lat, rl, emb = _inputs(5, f=F_)
    writer, reader = DR.write_banks(ref, den, rl, emb, F_, 16, 16)
    yield den, _two(lat), emb.half()
    reader.clear()
    writer.clear()
    den.clear_context_cache()
    ref.clear_context_cache()
    den.packed().pop("_two_queue_shapes", None)


def _call(den, x, emb, **kw):
    return DR.call_nhwc(den, x, T, emb, halves_identical=True, two_queues=True, **kw)


def _ran_two_lanes(den, slot):
    return (F_, 16, 16) in den.packed()["_two_queue_shapes"] and sorted(slot.store["bufs"]) == [0, 1]


@pytest.mark.parametrize("d", DEPTHS)
def test_two_lane_replay_is_bitwise_the_full_call(two_lanes, d):
    den, x, emb = two_lanes
    full = _call(den, x, emb)
    slot = DeepCacheSlot(d)
    n0 = len(fake_ops.CALLS)
    a = _call(den, x, emb, deep_cache=slot)
    n_fill = len(fake_ops.CALLS) - n0
    b = _call(den, x, emb, deep_cache=slot.reuse())
    n_reuse = len(fake_ops.CALLS) - n0 - n_fill
    c = _call(den, x, emb, deep_cache=slot.reuse())                        # the kept hidden states survive a reuse
    assert _ran_two_lanes(den, slot)
    assert torch.equal(a, full) and torch.equal(b, full) and torch.equal(c, full)
    assert n_reuse < n_fill / 3 * 2                                        # and it ran less
    assert full.isfinite().all()


@pytest.mark.parametrize("d", (1, 3))
def test_two_lane_auto_calls_are_their_forced_twins(two_lanes, d):
    """d = 1: a key step evaluates the shared first resnet between the phases; d = 3: down layers on both sides of the decision."""
    den, x, emb = two_lanes
    forced = DeepCacheSlot(d)
    fill = _call(den, x, emb, deep_cache=forced)
    reuse = _call(den, x, emb, deep_cache=forced.reuse())
    slot = DeepCacheSlot(d)
    first = _call(den, x, emb, deep_cache=slot.auto(math.inf, 2))         # an empty slot: a fill
    assert slot.last == "key" and slot.last_distance is None and torch.equal(first, fill)
    second = _call(den, x, emb, deep_cache=slot.auto(math.inf, 2))
    assert slot.last == "shallow" and slot.last_distance == 0.0           # the same inputs: the new skip IS the kept one
    assert torch.equal(second, reuse) and torch.equal(second, fill)
    assert _ran_two_lanes(den, slot) and _ran_two_lanes(den, forced)
    slot = DeepCacheSlot(d)
    for k in range(3):                                                     # max_run = 1: every call is a key step
        out = _call(den, x, emb, deep_cache=slot.auto(math.inf, 1))
        assert slot.last == "key" and torch.equal(out, fill), k
    assert _ran_two_lanes(den, slot)
    assert len([c for c in fake_ops.CALLS if c[0] == "rel_l1"]) == 2 * (1 + 2)      # one distance per lane of every call on a filled slot


def test_lane_one_is_the_conditional_call(two_lanes, monkeypatch):
    """forward_nhwc's docstring: conditional=True is the conditional queue of a two_queues call, launch for launch.
    The two calls take their time rows from GEMMs of 2 rows and of 1 row.  The emulated GEMM is torch's, whose CPU matmul sums a 1-row
    product in another order than a 2-row one (1.2e-4 on these time rows; on the MI355X the HIP GEMM's rows do not depend on their number
    and this comparison, unpatched, is bitwise: profiles/unet_lanes_refactor.json).  That is the emulator's property, not the schedule's:
    here every time-row GEMM runs on 2 rows and the call takes its own rows of it.  Everything else is as the calls issue it."""
    den, x5, emb = two_lanes
    real = den._time_rows
    monkeypatch.setattr(den, "_time_rows", lambda pk, ts, dev: real(pk, torch.full((2,), float(T)), dev)[2 - len(ts):], raising=False)
    b, c, f, hh, ww = x5.shape
    st = x5.stride()
    x = ops.pack_nhwc(x5, b * f, f, (st[0], st[2], st[1], st[3], st[4]), 0, c, 64, hh, ww)
    cross = den._cross(emb, [i // f for i in range(b * f)], x.device)
    t = torch.full((2,), float(T))
    slot = DeepCacheSlot(3)
    both = den.forward_nhwc(x, 2, f, t, cross, halves_identical=True, two_queues=True, deep_cache=slot).view(2 * f, hh, ww, 4)
    assert _ran_two_lanes(den, slot)
    cond = den.forward_nhwc(x[f:], 1, f, t[1:], cross.rows(f, 2 * f), conditional=True).view(f, hh, ww, 4)
    assert torch.equal(both[f:], cond)
    assert not torch.equal(both[:f], cond)                                 # and lane 0 is the other half


def test_key_step_at_depth_1_where_the_shared_first_resnet_writes_its_skip(monkeypatch):
    """A one-level UNet: down_blocks.0 has neither attention nor a motion module, so the first resnet shared between the clip-halves is its
    layer's last operator and pushes skip 1 itself.  A key step of an auto call at depth 1 evaluates it between the decision and the
    hand-over: the hand-over must still take the buffer of skip 0 (_Skips.hand_over finds it by index), or the step keeps the wrong one and
    the reuse call behind it starts from another hidden state."""
    from mikudance_amd.synth import synth_state_dict
    with torch.device("meta"):
        shapes = {k: v.shape for k, v in M.UNet3DConditionModel(sample_size=16, block_out_channels=(64,), cross_attention_dim=64).state_dict().items()}
    den = M.UNet3DConditionModel(sample_size=16, block_out_channels=(64,), cross_attention_dim=64)
    den.load_state_dict({k: v.half() for k, v in synth_state_dict(shapes, seed=7).items()})
    den = den.half()
    b0 = den.down_blocks[0]
    assert not b0.has_cross_attention and b0.motion_modules[0] is None and len(den._skip_plan()) == 3
    fake_ops.install(monkeypatch)
    AR.install(monkeypatch)
    lat, _, emb = _inputs(5)
    x, emb = _two(lat), emb.half()
    plain = DR.call_nhwc(den, x, T, emb, halves_identical=True)
    assert torch.equal(plain, DR.call_nhwc(den, x, T, emb))               # the shared layers are the literal ones
    slot = DeepCacheSlot(1)
    for want in ("key", "key", "shallow"):                                 # a fill on the empty slot, a decided key step, a shallow step
        out = DR.call_nhwc(den, x, T, emb, halves_identical=True, deep_cache=slot.auto(math.inf, 1 if want == "key" else 2))
        assert slot.last == want and torch.equal(out, plain), want
    assert torch.equal(DR.call_nhwc(den, x, T, emb, halves_identical=True, deep_cache=slot.reuse()), plain)
    assert sorted(slot.store["bufs"]) == [0] and slot.store["bufs"][0].shape[-1] == den._skip_plan()[0] + 64


def test_dead_tail_stops_behind_the_last_bank_write(small_cpu, monkeypatch):
    """skip_dead_tail with every block in write mode: the walk ends inside the last writer's attention, behind its bank write."""
    ref, _, _, _ = small_cpu
    fake_ops.install(monkeypatch)
    _, rl, emb = _inputs(5)
    g = rl.repeat(2, 1, 1, 1, 1).reshape(4, 22, 16, 16).half()
    ehs = emb.repeat((2, 1, 1)).half()
    writer = M.ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    blocks = ref.transformer_blocks_in_order()
    last = ref.up_blocks[-1].attentions[-1].transformer_blocks[0]
    written_at = []

    class Bank(list):
        def append(self, v):
            written_at.append(len(fake_ops.CALLS))
            list.append(self, v)

    last.bank = Bank()
    try:
        full = ref(g, torch.zeros((), dtype=torch.long), encoder_hidden_states=ehs, return_dict=False)[0]
        assert full is not None and written_at[0] < len(fake_ops.CALLS)   # the full walk goes on behind the write
        banks = [tb.bank[0].clone() for tb in blocks]
        for tb in blocks:
            del tb.bank[:]
        del fake_ops.CALLS[:], written_at[:]
        ref.skip_dead_tail = True
        out = ref(g, torch.zeros((), dtype=torch.long), encoder_hidden_states=ehs, return_dict=False)[0]
        assert out is None
        assert not any(tb.stop_after_bank for tb in blocks)
        assert written_at == [len(fake_ops.CALLS)]                         # no operator is logged behind the last writer's bank write
        assert all(len(tb.bank) == 1 and torch.equal(tb.bank[0], w) for tb, w in zip(blocks, banks))
    finally:
        ref.skip_dead_tail = False
        writer.clear()
        ref.clear_context_cache()
