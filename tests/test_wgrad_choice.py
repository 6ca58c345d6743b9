"""The weight-gradient selection rule (conv2d_wgrad_choose, conv2d_wgrad.hip) through its host query dvsr_conv2d_wgrad_geometry,
against rows recorded from the commit before the rule existed (tests/golden/wgrad_choice_parent.json: what that commit's
conv2d_wgrad_prepare / conv2d_wgrad_launch / launch_split3 chose, every kernel kind and both sides of every threshold -- 1000,
1024 and 4000 tiles x cout blocks x cin blocks, 2048 tiles, the 8-slot cap).  No device: the query launches nothing."""
import ctypes
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def answers():
    """Every golden row through the query and the workspace function, once.  (The rule's switches are read once per process,
    each at its first use: the rows were recorded under the defaults.)"""
    from dynavsr_amd import _lib as L
    switches = [name for name, _scope, _dflt, _doc in L.switches() if name.startswith("DVSR_WGRAD_")]   # the rule's, from the library's table
    assert len(switches) >= 6 and not [k for k in switches if k in os.environ], "the golden rows hold under the default switches"
    with open(os.path.join(GOLDEN, "wgrad_choice_parent.json")) as f:
        doc = json.load(f)
    out = []
    for row in doc["rows"]:
        r = dict(zip(doc["columns"], row))
        dense = r["Cin"] * r["H"] * r["W"]
        d = L.Conv2dDesc(0x10000000 + r["x_off"], None, None, None, None, 0x20000000 + r["gy_off"], r["N"], r["Cin"], 0, r["H"], r["W"],
                         r["Cout"], r["ks"], r["stride"], r["pad"], 0, 2 * r["gy_ps"], 1, dense + r["x_bs_extra"] if r["x_bs_extra"] else 0,
                         0, None, 0)
        geo = (ctypes.c_int * 8)()
        L.check(L.lib().dvsr_conv2d_wgrad_geometry(d, r["mode"], r["groups"], ctypes.byref(geo)), "dvsr_conv2d_wgrad_geometry")
        out.append((r, list(geo), L.lib().dvsr_conv2d_wgrad_workspace_bytes(d, r["groups"])))
    return out


def _tiles(r):
    ho, wo = ((r[k] + 2 * r["pad"] - r["ks"]) // r["stride"] + 1 for k in ("H", "W"))
    return -(-wo // 32) * -(-ho // 2) * r["N"]


def test_golden_rows_cover_every_kind_and_threshold_side(answers):
    rows = [r for r, _g, _w in answers]
    assert {(r["geo"][0], r["geo"][1]) for r in rows} == {(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0), (4, 1), (5, 0)}
    work = lambda r: _tiles(r) * r["geo"][6] * r["geo"][7]   # noqa: E731
    for what, val, edge, near in (
            ("fp32 row split", lambda r: work(r) if r["geo"][0] == 1 and r["ks"] == 3 else None, 1024, 0.1),
            ("split row split", lambda r: work(r) if r["geo"][0] in (4, 5) else None, 4000, 0.1),
            ("two workgroups per CU of the split's row split", lambda r: work(r) if r["geo"][:2] == [4, 1] else None, 1000, 0.1),
            ("two workgroups per CU of the simple kernel", lambda r: _tiles(r) if r["geo"][0] == 0 else None, 2048, 0.15),
            ("slot cap", lambda r: r["geo"][3], 8, 0.2)):
        vals = [v for v in map(val, rows) if v is not None]
        assert any(edge * (1 - near) <= v < edge for v in vals) and any(edge <= v < edge * (1 + near) for v in vals), what


def test_geometry_reproduces_the_parent(answers):
    bad = [(r, geo) for r, geo, _w in answers if geo != r["geo"]]
    assert not bad, bad[:5]


def test_workspace_covers_the_slots(answers):
    """[group][slot][tap][o][c] partial sums and [group][slot][o] bias sums over the 64-blocks of the grid, nslot slots."""
    for r, geo, ws in answers:
        nslot, nob, ncb = geo[4], geo[6], geo[7]
        need = r["groups"] * nslot * (r["ks"] ** 2 * nob * 64 * ncb * 64 + nob * 64) * 4
        assert ws >= need, (r, geo, ws, need)
