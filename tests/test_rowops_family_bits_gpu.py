"""The Adam and mixture-NLL entries of csrc/rowops.hip against the bits a build of the recorded commit gave
(tests/golden/rowops_family_bits.json, written by tools/record_rowops_bits.py; the runs are tests/rowops_family_bits.py's).

Each family is one kernel behind several entries, so comparing two entries with each other compares a kernel with itself; what
keeps results where they were is this record of the kernels the entries had BEFORE they were folded together.  An input whose hash
does not reproduce fails the test (the generators of tests/rowops_parity.py moved): the record would then prove nothing.  GPU only."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rowops_family_bits as fb                                     # noqa: E402
import rowops_parity as rp                                          # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(REPO, "tests", "golden", "rowops_family_bits.json")) as _f:
    RECORD = json.load(_f)
NLL = rp.nll_cases()


def _compare(got, want):
    assert got["name"] == want["name"]
    assert got["inputs"] == want["inputs"], f"{got['name']}: the inputs are not the recorded ones: " \
        f"{sorted(k for k in want['inputs'] if got['inputs'].get(k) != want['inputs'][k])}"
    assert sorted(got["outputs"]) == sorted(want["outputs"]), f"{got['name']}: not the recorded set of runs"
    diff = [f"{run}: {buf}" for run in sorted(want["outputs"]) for buf in sorted(set(want["outputs"][run]) | set(got["outputs"][run]))
            if got["outputs"][run].get(buf) != want["outputs"][run].get(buf)]
    assert not diff, f"{got['name']}: {len(diff)} output buffer(s) differ from the build of {RECORD['commit']}: {diff}"


def test_the_record_names_its_build_and_covers_both_tables():
    assert len(RECORD["commit"]) >= 7 and RECORD["hipcc_version"]
    assert [r["name"] for r in RECORD["adam"]] == [c["name"] for c in rp.adam_cases()]
    assert [r["name"] for r in RECORD["nll"]] == [c["name"] for c in NLL]
    runs = {f"{v}/{s}" for v in fb.adam_variants() for s in ("shadow", "no_shadow")}
    assert all(set(r["outputs"]) == runs for r in RECORD["adam"])


def test_adam_entries_give_the_recorded_bits():
    """pa_adam_step, pa_adam_step_guarded (control block included) and pa_adam_step_ext in five configurations, unguarded and guarded,
    and a skipped step, at n = 1, 3, 4, 5, 1027 and 2048 * 256 * 4 + 7, with and without the bf16 shadow: p, m, v, shadow, EMA, ctl."""
    got = fb.adam_records()
    assert len(got) == len(RECORD["adam"])
    for g, w in zip(got, RECORD["adam"]):
        _compare(g, w)


@pytest.mark.parametrize("k", range(len(NLL)), ids=[c["name"] for c in NLL])
def test_nll_entries_give_the_recorded_bits(k):
    """pa_mixture_nll_fwd_fin, pa_mixture_nll_fwd (row_lse, count, hits), pa_mixture_nll_bwd_up in eight forms, and the _ext pair with
    everything off and with eps 0.1 + [B, T] weights + token_nll."""
    _compare(fb.nll_record(NLL[k]), RECORD["nll"][k])
