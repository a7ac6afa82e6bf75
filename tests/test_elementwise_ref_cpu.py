"""CPU: the yardsticks of tests/test_elementwise_gpu.py hold without the kernels.  tests/elementwise_ref.py's layout references equal the
offset-arithmetic emulations of tests/fake_ops.py on every call form and resize case, its nearest rule is PyTorch's, LAYOUT_FORMS has a row
for every pack / unpack call of the package, step_case alternates the counters, and fake_ops' fp32 step emulations (with the APG / PAG forms
of apg_ref.py / pag_ref.py) stay within the step bound on the very inputs, seeds and shapes of the GPU file, the two large shapes included:
a correct fp32 evaluation passes the bound the kernels are held to."""
import collections
import glob
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import apg_ref
import elementwise_ref as E
import fake_ops
import pag_ref

FAKE = SimpleNamespace(cfg_ddim_step=fake_ops.cfg_ddim_step, cfg_multistep_step=fake_ops.cfg_multistep_step, cfg_apg_prepare=apg_ref.cfg_apg_prepare,
                       cfg_ddim_step_apg=apg_ref.cfg_ddim_step_apg, cfg_multistep_step_apg=apg_ref.cfg_multistep_step_apg,
                       cfg_ddim_step_pag=pag_ref.cfg_ddim_step_pag, cfg_multistep_step_pag=pag_ref.cfg_multistep_step_pag)
ROW_IDS = [f"{r['op']}-{r['site']}" for r in E.LAYOUT_FORMS]


# ---- 1. the layout references against fake_ops
def _sizes(row):
    return E.RESIZE_CASES if row["resize"] else [E.ODD + E.ODD]


@pytest.mark.parametrize("row", E.PACK_FORMS, ids=[r["site"] for r in E.PACK_FORMS])
def test_pack_reference_is_fake_ops(row):
    for dt in row["dtypes"]:
        for hin, win, ho, wo in _sizes(row):
            _, src = E.strided_tensor(row["layout"], row["ctot"], 2, 3, hin, win, E.DTYPES[dt], torch.Generator().manual_seed(hin * 100 + wo))
            n, f, strides = E.call_strides(row["layout"], src)
            want = E.pack_reference(src, row["layout"], row["c_begin"], row["c_count"], row["cpad"], ho, wo)
            got = fake_ops.pack_nhwc(src, n, f, strides, row["c_begin"], row["c_count"], row["cpad"], ho, wo, hin=hin, win=win)
            assert want.shape == (n, ho, wo, row["cpad"]) and torch.equal(E.bits(got), E.bits(want)), (row["site"], dt, hin, win, ho, wo)
            assert not want[..., row["c_count"]:].any() and want[..., :row["c_count"]].any()


@pytest.mark.parametrize("row", E.UNPACK_FORMS, ids=[r["site"] for r in E.UNPACK_FORMS])
def test_unpack_reference_is_fake_ops(row):
    h, w = E.ODD
    for dt in row["dtypes"]:
        g = torch.Generator().manual_seed(row["cpad"] + row["c_count"])
        wholes = [E.strided_tensor(row["layout"], row["ctot"], 2, 3, h, w, E.DTYPES[dt], -7.0) for _ in range(2)]
        n, f, strides = E.call_strides(row["layout"], wholes[0][1])
        src = torch.randn((n, h, w, row["cpad"]), generator=g).half()
        E.unpack_reference(src, wholes[0][1], row["layout"], row["c_count"])
        fake_ops.unpack_nhwc(src, wholes[1][1], n, f, strides, row["c_count"], h, w)
        assert torch.equal(wholes[0][0], wholes[1][0]) and (wholes[0][0] != -7.0).any() and (wholes[0][0][..., 0] == -7.0).all()


def test_round_trip_and_concat_reference():
    g = torch.Generator().manual_seed(4)
    _, x = E.strided_tensor("NCFHW", 4, 2, 3, 7, 5, torch.float32, g)
    p = E.pack_reference(x, "NCFHW", 0, 4, 64, 7, 5)
    y = torch.zeros(x.shape)
    E.unpack_reference(p, y, "NCFHW", 4)
    assert torch.equal(y, x.half().float())
    a, b = torch.randn((7, 5, 8), generator=g).half(), torch.randn((7, 5, 16), generator=g).half()
    assert torch.equal(E.concat_reference(a, b), fake_ops.concat_channels(a, b)) and torch.equal(E.concat_reference(a, b)[..., 8:], b)


@pytest.mark.parametrize("hin,win,ho,wo", E.RESIZE_CASES + [(16, 16, 4, 4), (96, 128, 48, 64), (12, 12, 3, 6)])
def test_nearest_rule_is_interpolate_nearest(hin, win, ho, wo):
    x = torch.arange(hin * win, dtype=torch.float32).view(1, 1, hin, win)
    want = F.interpolate(x, size=(ho, wo), mode="nearest")[0, 0]
    iy, ix = E.nearest_index(ho, hin), E.nearest_index(wo, win)
    assert torch.equal(x[0, 0][iy][:, ix], want)
    assert torch.equal(iy, fake_ops._nearest(ho, hin)) and torch.equal(ix, fake_ops._nearest(wo, win))


def test_resize_cases_cover_what_they_name():
    pairs = {(a, b) for hin, win, ho, wo in E.RESIZE_CASES for a, b in ((hin, ho), (win, wo))}
    assert {(16, 5), (16, 3), (9, 4), (7, 3), (5, 8), (7, 12), (3, 7)} <= pairs and any(c[:2] == c[2:] for c in E.RESIZE_CASES)
    assert any((c[0] > c[2]) != (c[1] > c[3]) for c in E.RESIZE_CASES)      # H and W scaled differently
    assert E.ODD[0] != E.ODD[1] and all(v % 8 for v in E.ODD)


def test_resize_cases_tell_floor_from_round():
    """Every resize case but the identity gathers other rows or columns under min(floor(y s + 0.5), n_in - 1): a nearest rule that rounds instead
    of flooring fails each of them, while the 16 -> 4 of tests/test_kernels_gpu.py::test_pack_unpack_concat (an integer ratio) cannot see it."""
    import numpy as np
    rounded = lambda n_out, n_in: [min(int(np.floor(np.float32(y) * (np.float32(n_in) / np.float32(n_out)) + np.float32(0.5))), n_in - 1)
                                   for y in range(n_out)]
    for hin, win, ho, wo in E.RESIZE_CASES:
        differs = rounded(ho, hin) != E.nearest_index(ho, hin).tolist() or rounded(wo, win) != E.nearest_index(wo, win).tolist()
        assert differs == ((hin, win) != (ho, wo)), (hin, win, ho, wo)
    assert rounded(4, 16) == E.nearest_index(4, 16).tolist() and rounded(8, 5) != E.nearest_index(8, 5).tolist()


def test_layout_forms_has_a_row_for_every_call_of_the_package():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mikudance_amd")
    found = collections.Counter()
    for path in sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)):
        for op in re.findall(r"\bops\.(pack|unpack)_nhwc\(", open(path).read()):
            found[(os.path.relpath(path, pkg), op)] += 1
    rows = collections.Counter((r["site"].split(":")[0], r["op"]) for r in E.LAYOUT_FORMS)
    assert found == rows, (found - rows, rows - found)
    assert len({(r["site"], r["op"]) for r in E.LAYOUT_FORMS}) == len(E.LAYOUT_FORMS) == 23


# ---- 2. step_case and the fp32 emulations under the step bound
@pytest.mark.parametrize("ftot", [1, 2, 3, 5, 16, 48])
def test_step_case_gives_neighbouring_frames_different_counters(ftot):
    for seed in range(20):
        for halves in (1, 2):
            c = E.step_case("plain", ftot, 6, halves, seed)
            assert set(c.cnt.tolist()) <= {1.0, 2.0, 3.0} and (c.cnt[1:] != c.cnt[:-1]).all() and (ftot < 3 or c.cnt[0] != c.cnt[-1])
            assert c.ns.shape == (halves, ftot, 6, 4) and c.pp.shape == c.hist.shape == c.mprev.shape == (ftot, 6, 4) and c.z.dtype == torch.float16
            again = E.step_case("plain", ftot, 6, halves, seed)
            assert torch.equal(c.ns, again.ns) and torch.equal(c.cnt, again.cnt)
            # the planes are counter x a prediction: per frame their size follows the counter
            if ftot >= 2:
                assert float((c.ns[0] / c.cnt.view(-1, 1, 1)).std()) == pytest.approx(0.7 if halves == 2 else 1.3, rel=0.5)


def _emulation_holds(flavour, kind, ftot, hw, halves, second_round_from=None):
    co = E._coefficients(kind)
    case = E.step_case(flavour, ftot, hw, halves, E.step_seed(flavour, ftot, hw, halves))
    got, h_got, extra = E.run_step(FAKE, case, kind, co)
    if flavour == "apg":
        assert (extra[0][:, 0] < 1).any()                                  # the cap is at work
    E.check_step("EMULATED_STEP", case, kind, got, h_got, *E.step_want(case, kind, co, extra), second_round_from=second_round_from)


@pytest.mark.parametrize("ftot,h,w", E.SMALL_STEP_CASES)
@pytest.mark.parametrize("kind", E.KINDS)
def test_plain_emulations_hold_the_step_bound_small(ftot, h, w, kind):
    for halves in (1, 2):
        _emulation_holds("plain", kind, ftot, h * w, halves)


@pytest.mark.parametrize("flavour,halves", E.LARGE_FLAVOURS)
@pytest.mark.parametrize("kind,ftot,h,w", E.LARGE_STEP_CASES)
def test_emulations_hold_the_step_bound_past_one_grid_round(kind, ftot, h, w, flavour, halves):
    per = 1 if kind.startswith("ddim") else 4
    assert ftot * h * w * 4 // per > E.ROUND and E.ROUND % (h * w * 4 // per) != 0
    _emulation_holds(flavour, kind, ftot, h * w, halves, second_round_from=E.ROUND * per)


@pytest.mark.parametrize("ftot,h,w", E.BOUNDARY_CASES)
def test_emulation_holds_the_step_bound_at_the_round_boundary(ftot, h, w):
    assert ftot * h * w * 4 - E.ROUND in (0, 64)
    _emulation_holds("plain", "ddim-eta", ftot, h * w, 2)


def test_accumulate_reference_is_fake_ops():
    f, ftot, hw = 4, 7, 5
    for halves in (1, 2):
        pred, ns, cnt = E.accumulate_case(f, ftot, hw, halves, 3)
        for window in ([5, 6, 0, 1], [2, -1, 4, 3]):
            want = E.accumulate_reference(pred, ns, cnt, window, f, halves)
            a, b = ns.clone(), cnt.clone()
            fake_ops.window_accumulate(pred, a, b, torch.tensor(window, dtype=torch.int32), f, ftot, hw, halves=halves)
            assert torch.equal(a, want[0]) and torch.equal(b, want[1]) and not torch.equal(a, ns)
