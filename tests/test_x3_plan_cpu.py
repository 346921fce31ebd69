"""The bf16x3 cut plan pinned without a GPU: the dry driver of tests/x3_plan_scenarios.py replays every scenario through
pa_gemm_split_plan(commit = 1) and every field of tests/golden/x3_plan.json - recorded on the GPU from the commit before the plan
functions existed - must come out equal: taken / declined, the counters, the status and every inner argument block.  Beyond the
golden fields, the context state each plan reports must be where the following call puts its first cut or image."""
import json

import pytest

import x3_plan_scenarios as X

SCENARIOS = X.scenarios()


@pytest.fixture(scope="module")
def lib():
    return X.load_lib(dry=True)


@pytest.fixture(scope="module")
def golden():
    with open(X.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS)
    for name, sc in SCENARIOS.items():
        assert [e["call"] for e in golden[name]] == [c[0] for c in sc["calls"]], name


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dry_run_gives_the_recorded_plan(lib, golden, name):
    got = X.dry_run(lib, SCENARIOS[name])
    want = golden[name]
    assert len(got) == len(want)
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ, first: {wrong[:2]}"


def test_the_scenarios_reach_every_path(lib):
    """What the issue's list asks the scenarios to reach, read off the plans themselves (so a scenario that silently stopped
    reaching its path fails here, not only the golden comparison)."""
    st, out = {}, {}
    for name, sc in SCENARIOS.items():
        st[name] = {}
        out[name] = X.dry_run(lib, sc, st[name])
    members = [(name, k, m) for name in st for k, ms in st[name].items() for m in ms]
    sources = {s for _, _, m in members if m["taken"] for s in m["source"]}
    assert sources == {"caller", "segment", "forward", "made", "cache", "cache_cut", "scratch"}
    modes = {m["mode"][i] for _, _, m in members if m["taken"] for i in range(3) if m["blocks"][i]}
    assert modes == {0, 1, 2, 3, 4}
    assert all(e["taken"] == 1 for e in out["layouts"] if e["call"] == "gemm")
    assert sum(e["declined"] for e in out["declines"] if e["call"] == "gemm") == 8
    # the declined deferred split-K asks the exact kernel for fewer slices than the caller did
    dd = [e for e in out["declined_deferred"] if e["call"] == "gemm"]
    assert [(e["declined"], e["inner"][0]["splitk"]) for e in dd] == [(1, 3), (1, 2), (0, 4)]
    # groups: both found, dY alone, X alone, neither
    grp = st["segment_retain"][7]
    assert [m["source"][:2] for m in grp] == [["segment", "forward"], ["segment", "scratch"], ["scratch", "forward"], ["scratch", "scratch"]]
    drops = [(m["drop_seg"], m["drop_fwd"]) for _, _, m in members]
    assert (1, 0) in drops and (1, 1) in drops and (0, 1) in drops
    assert any(m["long_closed"] for _, _, m in members)
    assert max(m["nkeepL"] for _, _, m in members) == 128 and max(m["nkeep"] for _, _, m in members) == 16
    assert [e["image"] for e in out["forward_129"] if e["call"] == "reserve"][-1] is None
    assert [e["image"] for e in out["segment_17"] if e["call"] == "reserve"][-1] is None
    assert sum(e["made_hits"] for e in out["reserve"] if e["call"] == "gemm") == 2
    assert sum(1 for e in out["reserve"] if e["call"] == "reserve" and e["image"] is None) == 2
    assert [e["rc"] for e in out["group_declines"] if e["call"] == "group"] == [-1, -1]
    # a group that found images and then declined counts none of them; the single call after it counts its own
    declined = out["segment_retain"][8]
    assert declined["call"] == "group" and declined["rc"] == -1 and declined["reused"] == 0 and out["segment_retain"][9]["reused"] == 2


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_reported_state_is_where_the_next_call_cuts(lib, name):
    """keep_off / long_off after a call are the offsets of what the next call puts into the scratch: its first cut lies at keep_off -
    or at long_off after the segment's images were dropped, at 0 after the forward's were too (a forward always cuts at long_off) -
    and a producer's image at keep_off.  The list lengths only change by the images the calls themselves report."""
    sc = SCENARIOS[name]
    states = {}
    out = X.dry_run(lib, sc, states)
    pos = None                                                  # state after the previous GEMM / reserve call of the same config bracket
    mode = 0
    for k, e in enumerate(out):
        if e["call"] == "config":
            mode, pos = e["mode"], None
        elif e["call"] == "reserve" and e["image"] is not None:
            end = e["image"][1] + X._img(*sc["calls"][k][2:4])
            if pos is not None:
                assert e["image"] == ["scratch", pos["keep_off"]], (k, e, pos)
                pos = dict(keep_off=end, long_off=end if mode == 3 else pos["long_off"])
            elif mode == 3:                                     # (a forward starts at 0; a segment starts behind the forward's images)
                assert e["image"] == ["scratch", 0]
                pos = dict(keep_off=end, long_off=end)
        elif e["call"] in ("gemm", "group"):
            ms = states[k]
            cuts = [m["off"][i] for m in ms if m["taken"] for i in range(3) if m["source"][i] == "scratch"]
            if cuts and pos is not None:
                first = 0 if ms[0]["drop_fwd"] else pos["long_off"] if (ms[0]["drop_seg"] or mode == 3) else pos["keep_off"]
                assert cuts[0] == first, (k, cuts, pos, ms[0])
                assert cuts == sorted(cuts)
            last = ms[-1]
            assert last["keep_off"] >= last["long_off"] and (mode != 3 or last["keep_off"] == last["long_off"])
            assert last["keep_off"] <= sc["scratch"]
            pos = dict(keep_off=last["keep_off"], long_off=last["long_off"])
