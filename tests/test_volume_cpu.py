"""The assembly volume without a GPU: the restatement of tests/volume_reference.py against its voxel
oracle, metric.plank_volume_counts and the stand-alone host program of tools/volume_host (the kernel's own core,
csrc/volume_core.h, built by the host compiler under AddressSanitizer + UBSan and run as its own process) against the
restatement, the scores, the consensus choice and the options.  Every comparison of counts is integer equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import volume_reference as R
from conftest import REPO
from plankassembly_amd import metric as M

END = R.END


@pytest.fixture(scope="module")
def table():
    a, b = R.case_table()
    return a, b, R.volume_counts(a, b)


def _hand(name):
    return next(c for c in R.hand_cases() if c[0] == name)


# ------------------------------------------------------------------------------------------------ restatement, oracle, host metric
def test_restatement_equals_the_voxel_oracle(table):
    a, b, want = table
    assert a.shape == (48, 132) and want.dtype == np.int64
    assert want[:, 6:].max() <= 8
    assert np.array_equal(want, R.voxel_counts(a, b, bits=5))
    pairs = [(3, 7), (0, 0), (47, 1), (7, 3)]
    assert np.array_equal(R.volume_counts(a, b, pairs), R.voxel_counts(a, b, pairs, bits=5))
    assert np.array_equal(R.volume_counts(a, None), R.voxel_counts(a, None, bits=5))


def test_the_table_checks_itself(table):
    """What the oracle alone has to show for the table to be worth comparing on."""
    a, b, _ = table
    c = R.voxel_counts(a, b, bits=5)
    n = len(c)
    overlapping = int((c[:, 1] > c[:, 0]).sum())
    partial = int(((c[:, 4] > 0) & (c[:, 4] < np.minimum(c[:, 0], c[:, 2]))).sum())
    apart = int(((c[:, 4] == 0) & (c[:, 6] > 0) & (c[:, 7] > 0)).sum())
    print("table", n, overlapping, partial, apart)
    assert 4 * overlapping >= n and 4 * partial >= n and apart >= 1
    assert np.array_equal(c[:, 4], c[:, 0] + c[:, 2] - c[:, 5])
    assert (c[:, 0] <= c[:, 1]).all() and (c[:, 5] >= np.maximum(c[:, 0], c[:, 2])).all()


def test_hand_cases_have_the_answers_worked_out_by_hand():
    cases = R.hand_cases()
    assert {"face_sharing_unit_cubes", "nested", "identical_sides", "same_plank_twice", "inverted_and_zero_extent", "empty_side_a",
            "clamped_at_2_40", "end_at_0", "end_at_5", "end_at_6", "end_at_11", "end_at_12", "end_at_None"} <= {c[0] for c in cases}
    for name, a, b, want in cases:
        got = R.volume_counts([a], None if b is None else [b])[0].tolist()
        assert got == want, name
        assert M.plank_volume_counts(a, b, END).tolist() == want, name
    s = R.scores(np.asarray(_hand("face_sharing_unit_cubes")[3]))
    assert s["volume_iou"] == 0.0
    s = R.scores(np.asarray(_hand("identical_sides")[3]))
    assert s["volume_iou"] == 1.0 and s["self_overlap_a"] == 0.0 and s["self_overlap_b"] == 0.0
    assert R.scores(np.asarray(_hand("same_plank_twice")[3]))["self_overlap_a"] == 0.5
    s = R.scores(np.asarray(_hand("nested")[3]))
    assert s["volume_iou"] == 24 / 1000 and s["volume_precision"] == 1.0 and s["volume_recall"] == 24 / 1000


def test_host_metric_equals_the_restatement(table):
    a, b, want = table
    for i in range(len(a)):
        got = M.plank_volume_counts(a[i], b[i], END)
        assert got.dtype == np.int64 and got.tolist() == want[i].tolist(), i
    assert M.plank_volume_counts(a[0], None, END).tolist() == R.volume_counts(a[:1], None)[0].tolist()
    A, B = R.ceiling_pairs()
    assert np.array_equal(np.stack([M.plank_volume_counts(A[i], B[i], END) for i in range(4)]), R.volume_counts(A, B))


def test_scores_are_the_numpy_formula_and_zero_at_zero_denominators(table):
    counts = np.concatenate((table[2], np.asarray([c[3] for c in R.hand_cases()], dtype=np.int64)))
    want = R.scores(counts)
    got_t = M.volume_scores(torch.from_numpy(counts))
    got_n = M.volume_scores(counts)
    assert sorted(want) == sorted(got_t) == sorted(got_n)
    for k, w in want.items():
        assert got_t[k].dtype == torch.float64 and isinstance(got_n[k], np.ndarray)
        assert np.array_equal(got_t[k].numpy().view(np.int64), w.view(np.int64)), k
        assert np.array_equal(got_n[k].view(np.int64), w.view(np.int64)), k
    zero = M.volume_scores(torch.zeros(3, 8, dtype=torch.int64))
    assert all(bool((v == 0).all()) and bool(torch.isfinite(v).all()) for v in zero.values())
    one_side = M.volume_scores(np.asarray(_hand("empty_side_a")[3]))
    assert one_side["volume_iou"] == 0.0 and one_side["volume_recall"] == 0.0 and one_side["self_overlap_a"] == 0.0


# ------------------------------------------------------------------------------------------- the host program (csrc/volume_core.h)
def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found (set CXX)")


@pytest.fixture(scope="module")
def volume_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("volume_host") / "volume_host")
    src = os.path.join(REPO, "tools", "volume_host", "main.cpp")
    r = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_host(exe, tmp_path, a, b, pairs=None):
    if pairs is None:
        pairs = [(i, i) for i in range(len(a))]
    lines = [f"{len(pairs)} {END} 6"]
    for i, j in pairs:
        lines.append(" ".join([str(len(a[i]))] + [str(int(v)) for v in a[i]]))
        lines.append("-1" if b is None else " ".join([str(len(b[j]))] + [str(int(v)) for v in b[j]]))
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return np.asarray([[int(v) for v in ln.split()] for ln in r.stdout.splitlines()], dtype=np.int64).reshape(-1, 8)


def test_host_program_equals_the_restatement(volume_host, tmp_path, table):
    a, b, want = table
    assert np.array_equal(_run_host(volume_host, tmp_path, a, b), want)
    assert np.array_equal(_run_host(volume_host, tmp_path, a, None), R.volume_counts(a, None))
    for name, ra, rb, answer in R.hand_cases():
        assert _run_host(volume_host, tmp_path, [ra], None if rb is None else [rb])[0].tolist() == answer, name
    short = [np.zeros(n, dtype=np.int64) for n in (0, 1, 5, 6, 7, 12)]                # rows too short to hold a plank behind plank 0
    assert not _run_host(volume_host, tmp_path, short, short).any()


def test_host_program_at_170_planks_a_side(volume_host, tmp_path):
    a, b = R.ceiling_pairs()
    assert a.shape == (4, 1026)
    want = R.volume_counts(a, b)
    assert want[:, 6].tolist() == [170] * 4 and want[:, 7].tolist() == [170, 170, 170, 0]
    assert want[1, 0] == want[1, 1] and want[2, 1] == 170 * want[2, 0]               # all disjoint; all identical
    assert np.array_equal(_run_host(volume_host, tmp_path, a, b), want)


def test_host_program_refuses_what_the_library_refuses(volume_host, tmp_path):
    row = "6 0 0 0 1 1 1\n"
    for text in ("1 512 4\n" + row + row, "1 512 6\n1027 " + "1 " * 1027 + "\n" + row, "1 512 6\n" + row + "1027 " + "1 " * 1027 + "\n",
                 "1 512 6\n-1\n" + row, "1 512 6\n" + row + "-2\n", "-1 512 6\n"):
        path = os.path.join(str(tmp_path), "bad.txt")
        with open(path, "w") as f:
            f.write(text)
        r = subprocess.run([volume_host, path], capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.strip() == "error", text[:40]
    path = os.path.join(str(tmp_path), "none.txt")
    with open(path, "w") as f:
        f.write("0 512 6\n")
    r = subprocess.run([volume_host, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""


# ------------------------------------------------------------------------------------------------------------- the consensus
def _select_cpu(sample_rows):
    """decode._pick_volume on torch CPU, the counts from the restatement: sample_rows [B][N] token rows."""
    from plankassembly_amd.decode import _pick_volume
    N = len(sample_rows[0])
    iu = torch.triu_indices(N, N, 1)
    counts = np.stack([R.volume_counts(rows, rows, list(zip(iu[0].tolist(), iu[1].tolist()))) for rows in sample_rows])
    return _pick_volume(torch.from_numpy(counts), N, iu[0], iu[1]), counts


def test_volume_select_breaks_ties_towards_the_lower_index():
    x = R.row_of([(0, 0, 0, 4, 4, 4), (2, 2, 2, 8, 8, 8)], 36)
    y = R.row_of([(1, 1, 1, 5, 5, 5)], 36)
    z = R.row_of([(20, 20, 20, 22, 22, 22)], 36)
    e = R.row_of([], 36)
    got, counts = _select_cpu([[y, x, x, z], [x, x, x, x], [e, e, z, e], [z, y, x, y], [e, e, e, e]])
    index, mean = R.select(counts, 4)
    assert got["volume_index"].dtype == torch.int64 and got["volume_index"].tolist() == index.tolist() == [1, 0, 0, 1, 0]
    assert got["volume_iou"].dtype == torch.float64 and np.array_equal(got["volume_iou"].numpy().view(np.int64), mean.view(np.int64))
    u = got["volume_iou"].numpy()
    assert u[0, 1] == u[0, 2] and u[1].tolist() == [1.0] * 4
    assert u[2].tolist() == [0.0] * 4 and u[4].tolist() == [0.0] * 4                   # two that occupy nothing: IoU 0
    own = R.scores(R.volume_counts([y, x, x, z], None))["self_overlap_a"]
    assert np.array_equal(got["self_overlap"][0].numpy().view(np.int64), own.view(np.int64)) and own[1] > 0.0 == own[0]
    # graded where the plank F1 has nothing to rank: no two samples share a plank at IoU > 0.5, the utilities still differ
    p = [R.row_of([(0, 0, 0, 10, 10, 10 + 4 * k)], 36) for k in range(4)]
    got, counts = _select_cpu([p])
    assert got["volume_index"].tolist() == R.select(counts, 4)[0].tolist() and len(set(got["volume_iou"][0].tolist())) > 1


# ----------------------------------------------------------------------------------------------------------------- the options
def test_check_select_accepts_volume_and_nothing_else():
    from plankassembly_amd.models import PlankModel
    assert PlankModel._check_select("volume") == "volume"
    assert PlankModel._check_select("consensus") == "consensus" and PlankModel._check_select("reprojection") == "reprojection"
    assert PlankModel._check_select(None) is None
    with pytest.raises(ValueError):
        PlankModel._check_select("median")


def _trainer(model=None, data=None, cls=None, **hparams):
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import Trainer
    _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_complete.yaml"))
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=1, NUM_DECODER_LAYERS=1, **(model or {}))
    hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36, **(data or {}))
    hp.update(hparams)
    return (cls or Trainer)(hp)


def test_build_model_reads_sample_select_volume():
    t = _trainer()
    assert t.model.sample_select is None and t.volume_metric is False
    t = _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="volume", SHARE_ENCODER=True, CONSTRAIN_PLANKS=True))
    assert t.model.sample_select == "volume"
    for model in (dict(SAMPLE_SELECT="volume"), dict(SAMPLE_SELECT="volume", BEAM_SIZE=4),
                  dict(NUM_SAMPLES=4, SAMPLE_SELECT="volume", BEAM_SIZE=2), dict(NUM_SAMPLES=4, SAMPLE_SELECT="volumes"),
                  dict(NUM_SAMPLES=4, SAMPLE_SELECT=3)):
        with pytest.raises(ValueError):
            _trainer(model)
    with pytest.raises(ValueError):                                                  # planks of six DOF only
        _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="volume"), dict(NUM_OUTPUT_DOF=4))


def test_volume_metric_is_a_validated_hparam():
    from plankassembly_amd.trainer import SidefaceTrainer, volume_option
    assert _trainer(VOLUME_METRIC=True).volume_metric is True
    assert _trainer(VOLUME_METRIC=False).volume_metric is False
    assert _trainer(cls=SidefaceTrainer, VOLUME_METRIC=True).volume_metric is True    # any input kind
    assert volume_option({}) is False
    for v in ("true", 1, "yes", 0.5):
        with pytest.raises(ValueError):
            _trainer(VOLUME_METRIC=v)
    with pytest.raises(ValueError):
        volume_option({"VOLUME_METRIC": True}, 4)
    with pytest.raises(ValueError):
        _trainer(data=dict(NUM_OUTPUT_DOF=4), VOLUME_METRIC=True)
    assert volume_option({"VOLUME_METRIC": False}, 4) is False


def test_the_entry_is_declared_bound_and_built():
    from plankassembly_amd import build
    assert "volume.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "volume.hip")) and os.path.exists(os.path.join(build.CSRC, "volume_core.h"))
    header = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    m = re.search(r"int pa_plank_volume\(([^;]*)\);", header)
    assert m and m.group(1).count(",") == 12                                          # 13 arguments
    lib_py = open(os.path.join(REPO, "plankassembly_amd", "_lib.py")).read()
    m = re.search(r'"pa_plank_volume": \(I, \[([^\]]*)\]\)', lib_py)
    assert m and m.group(1).count(",") == 12
