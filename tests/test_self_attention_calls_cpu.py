"""CPU: the operator calls of one TransformerBlock in every way its self-attention can differ from the plain one, pinned against a recording.

tests/golden/self_attention_calls.json holds, for every case of MODES x POOLS, the sequence of operator calls the block issued BEFORE the
four channels pag= / seg= / kv_pool= / the clip-half module global became one blocks.SelfAttnCall: every call's name, every tensor argument's
dtype, shape, strides and storage offset (and the packed weight's name where it is one), and every scalar argument that is not at its
default.  The block must still issue exactly those.  One difference is permitted: ops.token_blur reads and writes q alone, so its entry is
compared for its arguments and for lying behind the GEMM that made q and in front of the attention launch, not for its place among
token_pool and the k / v^T GEMMs.

The recording was made at the parent commit with this module and the old spelling of the one call:

    import json, pytest, test_self_attention_calls_cpu as t
    from mikudance_amd import blocks
    def old(blk, h, B, L, cross, half, pert, pool):
        kw = {} if pool is None else dict(kv_pool=(t.HH, t.WW) + pool)
        if pert is not None and pert[0] == "identity":
            kw["pag"] = pert[1]
        if pert is not None and pert[0] == "blur":
            kw["seg"] = (pert[1], t.HH, t.WW, pert[2])
        blocks.CHAIN = half
        try:
            return blk(h, B, L, cross, **kw)
        finally:
            blocks.CHAIN = None
    with pytest.MonkeyPatch.context() as mp:
        got = {kind: t.trace_all(mp, kind, old) for kind in ("2d", "3d")}
    assert got["2d"] == got["3d"]
    json.dump(t.pack(got["2d"]), open(t.GOLDEN, "w"), indent=0)

tests/golden/self_attention_option_calls.json is a second recording, of what the block issued BEFORE its two projection paths (the plain one in
TransformerBlock.forward and the tile-major one beside it) became one method: at the grids of GRIDS -- 8 x 8, where a t = 2 tile holds
Lt = 16 tokens (the fused tiled path), and 4 x 6, where it holds Lt = 6, roundup8(Lt) != Lt (the unfused padded path; plain L = 24) -- every
block state of STATES under every option set of OPTIONS (none, pool, tile, tile + pool), and the perturbed evaluation under every entry of
PERTURBED.  Per call it holds what the first recording holds and, behind "alias=", the pairs of tensor arguments that share their storage
(the q | k halves of the fused GEMM's output, an in-place `out=`).  The block must issue exactly those, in that order: nothing is permitted
to differ.  It was made at the parent commit with this module as it is:

    import test_self_attention_calls_cpu as t
    t.dump_options()
"""
import inspect
import json
import math
import os

import pytest
import torch

from mikudance_amd import blocks, ops

import fake_ops
import todo_ref as T

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "self_attention_calls.json")
HH, WW, F, DIM = 4, 4, 2, 64
POOLS = {"none": None, "nearest": (2, "nearest"), "mean": (2, "mean")}
# mode -> (ref_mode, ref_cfg, stop_after_bank, rows of the CFG batch ("all" / "uncond" / "cond"), clip-half, perturbation)
#   perturbation: None, ("identity", selected?) or ("blur", selected?, sigma)
MODES = {"plain": (None, False, False, "all", None, None),
         "write": ("write", False, False, "all", None, None),
         "write-stop": ("write", False, True, "all", None, None),
         "read": ("read", False, False, "cond", None, None),
         "read-cfg": ("read", True, False, "all", None, None),
         "read-cfg-uncond": ("read", True, False, "uncond", 0, None),
         "read-cfg-cond": ("read", True, False, "cond", 1, None),
         "identity-selected": ("read", True, False, "cond", None, ("identity", True)),
         "perturbed-unselected": ("read", True, False, "cond", None, ("identity", False)),
         "blur-1.5": ("read", True, False, "cond", None, ("blur", True, 1.5)),
         "blur-inf": ("read", True, False, "cond", None, ("blur", True, math.inf))}


def block_call(blk, h, B, L, cross, half, pert, pool):
    """The one call whose spelling changed: pert is None, ("identity", blocks) or ("blur", blocks, sigma); pool None or (s, mode)."""
    sa = blocks.SelfAttnCall(half=half, identity=pert[1] if pert is not None and pert[0] == "identity" else None,
                             blur=pert[1:] if pert is not None and pert[0] == "blur" else None, pool=None if pool is None else {blk: pool})
    return blk(h, B, L, cross, sa=sa, grid=(HH, WW))


def _describe(v, names):
    if isinstance(v, torch.Tensor):
        s = f"{str(v.dtype)[6:]}{list(v.shape)}s{list(v.stride())}+{v.storage_offset()}"
        return f"{names[id(v)]}:{s}" if id(v) in names else s
    return repr(v)


def _recorded(name, fn, log, names, aliases=False):
    """fn, logging "name(arg=..., ...)" of every call: the arguments by name, those left at or given their default omitted.  aliases: followed
    by " alias=a~b,..." where two tensor arguments share their storage."""
    params = inspect.signature(fn).parameters

    def wrapper(*a, **kw):
        given = inspect.signature(fn).bind(*a, **kw).arguments
        rec = name + "(" + ", ".join(f"{k}={_describe(v, names)}" for k, v in given.items()
                                     if isinstance(v, torch.Tensor) or not (v is params[k].default or v == params[k].default)) + ")"
        if aliases:
            ts = [(k, v.untyped_storage().data_ptr()) for k, v in given.items() if isinstance(v, torch.Tensor)]
            pairs = [f"{a_}~{b_}" for i, (a_, pa) in enumerate(ts) for b_, pb in ts[i + 1:] if pa == pb]
            rec += " alias=" + ",".join(pairs) if pairs else ""
        log.append(rec)
        return fn(*a, **kw)
    return wrapper


def trace_all(monkeypatch, kind, call):
    """{"mode/pool": [call, ...]} of the block of todo_ref.block_setup under the emulated operators, each case from a block with nothing cached."""
    fake_ops.install(monkeypatch)
    st = T.block_setup(DIM, DIM, HH, WW, F, torch.device("cpu"))
    blk, L = st.blk, st.L
    blk.kind = kind
    log, names = [], {id(v): k for k, v in blk.packed().items() if isinstance(v, torch.Tensor)}
    for name in [n for n in fake_ops._NAMES if n != "require_gpu"] + ["token_pool", "token_blur"]:
        monkeypatch.setattr(ops, name, _recorded(name, getattr(ops, name), log, names))
    h = st.x.reshape(2 * F * L, DIM)
    rows = {"all": (0, 2 * F), "uncond": (0, F), "cond": (F, 2 * F)}
    out = {}
    with torch.no_grad():
        for mode, (ref_mode, cfg, stop, which, half, pert) in MODES.items():
            for pname, pool in POOLS.items():
                lo, hi = rows[which]
                blk.ref_mode, blk.ref_cfg, blk.stop_after_bank, blk._kv_cache = ref_mode, cfg, stop, None
                blk.bank = [st.bank] if ref_mode == "read" else []
                sel = None if pert is None else (pert[0], (blk,) if pert[1] else ()) + pert[2:]
                del log[:]
                call(blk, h[lo * L:hi * L].clone(), hi - lo, L, st.cross if which == "all" else st.cross.rows(lo, hi), half, sel, pool)
                out[f"{mode}/{pname}"] = list(log)
    blk.ref_mode, blk.ref_cfg, blk.stop_after_bank, blk.bank = None, False, False, []
    return out


def pack(traces):
    """The traces with every distinct call written once: {"calls": [...], "cases": {case: [index, ...]}}."""
    calls = sorted({c for seq in traces.values() for c in seq})
    return {"calls": calls, "cases": {k: [calls.index(c) for c in seq] for k, seq in traces.items()}}


def unpack(packed):
    return {k: [packed["calls"][i] for i in seq] for k, seq in packed["cases"].items()}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return unpack(json.load(fh))


@pytest.mark.parametrize("kind", ["2d", "3d"])
def test_block_issues_the_recorded_calls(monkeypatch, recorded, kind):
    got = trace_all(monkeypatch, kind, block_call)
    assert sorted(got) == sorted(recorded) and len(got) == len(MODES) * len(POOLS)
    for case, want in recorded.items():
        seq = got[case]
        blur_w, blur_g = [c for c in want if c.startswith("token_blur(")], [c for c in seq if c.startswith("token_blur(")]
        assert blur_g == blur_w and len(blur_w) == (1 if case.startswith("blur-") else 0), case
        assert [c for c in seq if c not in blur_g] == [c for c in want if c not in blur_w], case
        if blur_g:
            at = seq.index(blur_g[0])
            made_q = [i for i, c in enumerate(seq) if c.startswith("gemm(") and "w=q1:" in c]
            attn = [i for i, c in enumerate(seq) if c.startswith("attention(")]
            assert len(made_q) == 1 and made_q[0] < at < attn[0], case


def test_refused_combinations(monkeypatch):
    fake_ops.install(monkeypatch)
    st = T.block_setup(DIM, DIM, HH, WW, F, torch.device("cpu"))
    blk, L = st.blk, st.L
    h, cross = st.x[F:].reshape(F * L, DIM), st.cross.rows(F, 2 * F)
    for half in (0, 1):                                                    # a perturbed evaluation as a clip-half
        with pytest.raises(ValueError, match="perturbed evaluation is a call of its own"):
            blocks.SelfAttnCall(half=half, identity=(blk,))
        with pytest.raises(ValueError, match="perturbed evaluation is a call of its own"):
            blocks.SelfAttnCall(half=half, blur=((blk,), 1.5))
    with pytest.raises(ValueError, match="two perturbations of one evaluation"):
        blocks.SelfAttnCall(identity=(blk,), blur=((blk,), 1.5))
    blk.ref_mode = "write"                                                 # a perturbed evaluation that writes the bank
    for sa in (blocks.SelfAttnCall(identity=(blk,)), blocks.SelfAttnCall(identity=()), blocks.SelfAttnCall(blur=((blk,), 1.5))):
        with pytest.raises(ValueError, match="not a bank write"):
            blk(h.clone(), F, L, cross, sa=sa, grid=(HH, WW))
    assert blk.bank == []
    blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank]
    for sa in (blocks.SelfAttnCall(pool={blk: (2, "nearest")}), blocks.SelfAttnCall(blur=((blk,), 1.5))):   # a grid that does not hold L
        for grid in ((HH, WW + 1), None):
            with pytest.raises(ValueError, match=f"does not hold L = {L}"):
                blk(h.clone(), F, L, cross, sa=sa, grid=grid)
    blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []


# ------------------------------------------------------------------ the second recording: every option set at two grids
OPTION_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "self_attention_option_calls.json")
GRIDS = {"8x8": (8, 8), "4x6": (4, 6)}
POOL, TILE, SIGMA = (2, "mean"), (2, (1, 1)), 1.5
# state -> (ref_mode, ref_cfg, stop_after_bank, rows of the CFG batch, clip-half)
STATES = {"plain": (None, False, False, "all", None),
          "write": ("write", False, False, "all", None),
          "write-stop": ("write", False, True, "all", None),
          "read": ("read", False, False, "cond", None),
          "read-cfg": ("read", True, False, "all", None),
          "half0": ("read", True, False, "uncond", 0),
          "half1": ("read", True, False, "cond", 1)}
OPTIONS = {"none": (None, None), "pool": (POOL, None), "tile": (None, TILE), "tile+pool": (POOL, TILE)}     # (pool, tile)
# the perturbed evaluation (read + ref_cfg, the conditional rows, every row reads the bank): (perturbation, pool, tile)
PERTURBED = {"identity": ("identity", None, None), "blur": ("blur", None, None), "blur+pool": ("blur", POOL, None), "blur+tile": ("blur", None, TILE),
             "blur+tile+pool": ("blur", POOL, TILE), "identity+pool+tile": ("identity", POOL, TILE)}


def trace_options(monkeypatch):
    """{"grid/state/options" and "grid/perturbed/entry": [call, ...]} of the block of todo_ref.block_setup under the emulated operators."""
    import tile_ref
    fake_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "token_tile", tile_ref.token_tile, raising=False)
    monkeypatch.setattr(ops, "token_untile", tile_ref.token_untile, raising=False)
    log, names = [], {}
    for name in [n for n in fake_ops._NAMES if n != "require_gpu"] + ["token_pool", "token_blur", "token_tile", "token_untile"]:
        monkeypatch.setattr(ops, name, _recorded(name, getattr(ops, name), log, names, aliases=True))
    out = {}
    with torch.no_grad():
        for gname, grid in GRIDS.items():
            st = T.block_setup(DIM, DIM, grid[0], grid[1], F, torch.device("cpu"))
            blk, L = st.blk, st.L
            names.clear()
            names.update({id(v): k for k, v in blk.packed().items() if isinstance(v, torch.Tensor)})
            h = st.x.reshape(2 * F * L, DIM)
            rows = {"all": (0, 2 * F), "uncond": (0, F), "cond": (F, 2 * F)}

            def run(case, ref_mode, cfg, stop, which, sa):
                lo, hi = rows[which]
                blk.ref_mode, blk.ref_cfg, blk.stop_after_bank, blk._kv_cache = ref_mode, cfg, stop, None
                blk.bank = [st.bank] if ref_mode == "read" else []
                del log[:]
                blk(h[lo * L:hi * L].clone(), hi - lo, L, st.cross if which == "all" else st.cross.rows(lo, hi), sa=sa, grid=grid)
                out[f"{gname}/{case}"] = list(log)

            for state, (ref_mode, cfg, stop, which, half) in STATES.items():
                for oname, (pool, tile) in OPTIONS.items():
                    run(f"{state}/{oname}", ref_mode, cfg, stop, which,
                        blocks.SelfAttnCall(half=half, pool=pool and {blk: pool}, tile=tile and {blk: tile}))
            for pname, (pert, pool, tile) in PERTURBED.items():
                run(f"perturbed/{pname}", "read", True, False, "cond",
                    blocks.SelfAttnCall(identity=(blk,) if pert == "identity" else None, blur=((blk,), SIGMA) if pert == "blur" else None,
                                        pool=pool and {blk: pool}, tile=tile and {blk: tile}))
            blk.ref_mode, blk.ref_cfg, blk.stop_after_bank, blk.bank = None, False, False, []
    return out


def dump_options(path=OPTION_GOLDEN):
    with pytest.MonkeyPatch.context() as mp:
        got = trace_options(mp)
    with open(path, "w") as fh:
        json.dump(pack(got), fh, indent=0)


@pytest.fixture(scope="module")
def option_traces():
    with pytest.MonkeyPatch.context() as mp:
        got = trace_options(mp)
    with open(OPTION_GOLDEN) as fh:
        return got, unpack(json.load(fh))


OPTION_CASES = [f"{g}/{s}/{o}" for g in GRIDS for s in STATES for o in OPTIONS] + [f"{g}/perturbed/{p}" for g in GRIDS for p in PERTURBED]


def test_the_option_recording_holds_every_case_and_no_other(option_traces):
    got, want = option_traces
    assert sorted(want) == sorted(OPTION_CASES) == sorted(got)
    for g in GRIDS:
        assert want[f"{g}/perturbed/identity+pool+tile"] == want[f"{g}/perturbed/identity"]          # no attention to shorten or to tile
        assert not any(c.startswith(("attention(q=float16[", "token_")) and "kv_index" not in c for c in want[f"{g}/perturbed/identity"])
    # the two tiled paths: 8 x 8 fuses q | k behind ONE reorder, 4 x 6 (Lt = 6) reorders q and the padded K / V source on their own
    fused, padded = want["8x8/plain/tile"], want["4x6/plain/tile"]
    assert len([c for c in fused if c.startswith("token_tile(")]) == 1 and any("w=qk1:" in c for c in fused)
    assert len([c for c in padded if c.startswith("token_tile(")]) == 2 and not any("w=qk1:" in c for c in padded)
    assert any(c.startswith("token_tile(") and "tile_stride=8" in c for c in padded)


@pytest.mark.parametrize("case", OPTION_CASES)
def test_block_issues_the_recorded_option_calls(option_traces, case):
    got, want = option_traces
    assert got[case] == want[case], case
