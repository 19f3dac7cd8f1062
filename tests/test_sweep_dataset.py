"""CPU suite: the sweep and the score at dataset scale - IIW splits (whdr.iiw_split against the lists
the reference's own functions return, tests/golden/iiw_split.json), --split / --report_split of the
two tools, and one process per rank (sweep.run_sharded) over real gloo groups of 2 and 3 ranks on
localhost.  The device work is stood in for by tests/sweep_stubs.py: every per-photo value is a
function of the file name, so a merge that drops, repeats or reorders a photo shows.  The files
written at world size 2 and 3 are compared with those of one process: the JSON byte for byte, the npz
array for array.
"""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from reflectance_filtering_amd import score as score_cli
from reflectance_filtering_amd import sharding
from reflectance_filtering_amd import sweep as sweep_cli
from reflectance_filtering_amd import whdr
from tests import sweep_stubs as stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "iiw_split.json")
TODAY = ["filter_type", "guidance", "delta", "sigma_color", "sigma_spatial", "pairs", "mean_whdr",
         "best", "images", "images_with_judgements"]
GRID = ["--sigma_color", "20,7", "--sigma_spatial", "1.5,3"]
PAIRS = [[20.0, 1.5], [20.0, 3.0], [7.0, 1.5], [7.0, 3.0]]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _touch(folder, stems):
    """Empty `<stem>.png` files (the stand-ins never read them): their names, in the order given."""
    folder.mkdir(exist_ok=True)
    names = []
    for stem in stems:
        name = str(folder / (stem + ".png"))
        open(name, "w").close()
        names.append(name)
    return names


# ---- the splits -------------------------------------------------------------------------------------------

def test_the_fixture_holds_what_the_issue_asks_of_it(golden):
    stems = golden["stems"]
    assert len(stems) >= 120 and len(set(stems)) == len(stems)
    assert {"9", "10", "100", "10-x"} <= set(stems)
    assert any(ord(ch) > 127 for stem in stems for ch in stem)
    assert stems != sorted(stems)
    assert len(golden["big_train_mini_val"]["val"]) == 2        # positions 6 and 106


@pytest.mark.parametrize("scheme", whdr.SPLIT_SCHEMES)
def test_iiw_split_equals_the_references_lists(golden, scheme):
    stems = golden["stems"]
    split = whdr.iiw_split(stems, scheme)
    assert sorted(split) == sorted(golden[scheme])
    assert ("val" in split) == (scheme != "train_test")
    for name, index in split.items():
        assert [stems[i] for i in index] == golden[scheme][name], name
    assert sorted(i for index in split.values() for i in index) == list(range(len(stems)))
    # the order the list is given in does not matter
    again = whdr.iiw_split(stems[::-1], scheme)
    for name, index in again.items():
        assert [stems[::-1][i] for i in index] == golden[scheme][name], name


def test_the_position_is_that_of_the_stem_not_of_the_path(tmp_path):
    # as paths: 10-x.png < 10.png < 100.png < 11.png < 9.png; as stems: 10 < 10-x < 100 < 11 < 9
    photos = sweep_cli.select_split
    names = _touch(tmp_path / "iiw", ["10-x", "10", "100", "11", "9", "12"])
    from reflectance_filtering_amd.batch import expand_inputs
    listed = expand_inputs([str(tmp_path / "iiw" / "*.png")])
    assert [sweep_cli.stem_of(f) for f in listed] == ["10-x", "10", "100", "11", "12", "9"]
    assert sorted(sweep_cli.stem_of(f) for f in listed) == ["10", "10-x", "100", "11", "12", "9"]
    test, info = photos(listed, "test", "train_test")
    assert [sweep_cli.stem_of(f) for f in test] == ["10", "9"]        # positions 0 and 5 of the stems
    assert info == {"name": "test", "scheme": "train_test", "of": 6, "images": 2}
    train, _ = photos(listed, "train", "train_test")
    assert [sweep_cli.stem_of(f) for f in train] == ["10-x", "100", "11", "12"]
    assert photos(names, "all", "train_test") == (names, None)
    assert whdr.iiw_split(["10-x", "10"], "train_test") == {"test": [1], "train": [0]}


def test_duplicate_stems_are_refused_by_name(tmp_path):
    with pytest.raises(ValueError) as err:
        whdr.iiw_split(["7", "8", "7"], "train_test")
    assert "'7'" in str(err.value) and "0" in str(err.value) and "2" in str(err.value)
    a, b = str(tmp_path / "a" / "10.png"), str(tmp_path / "b" / "10.jpg")
    with pytest.raises(ValueError) as err:
        sweep_cli.select_split([a, str(tmp_path / "a" / "11.png"), b], "test", "train_val_test")
    assert a in str(err.value) and b in str(err.value)
    with pytest.raises(ValueError):
        whdr.iiw_split(["1"], "narihira")


# ---- the command line, in this process --------------------------------------------------------------------

def _sweep_argv(folder, out, extra=()):
    return (["--inputs", str(folder / "*.png"), "--filter_type", "guided"] + GRID
            + ["--out", str(out / "sweep.json"), "--per_image", str(out / "sweep.npz")] + list(extra))


def _want_mean(photos, pairs, k=0):
    judged = [f for f in photos if stubs.judged(f)]
    return np.array([[stubs.value(f, pair, k) for f in judged] for pair in pairs]).mean(axis=1)


def test_split_all_writes_exactly_the_keys_of_before(tmp_path, monkeypatch, capsys):
    stubs.install(monkeypatch.setattr)
    photos = sorted(_touch(tmp_path / "iiw", ["%d" % i for i in range(1, 24)]))
    assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "all"])) == 0
    with open(str(tmp_path / "sweep.json")) as fh:
        text = fh.read()
    result = json.loads(text)
    assert list(result) == TODAY
    pairs, per_image, has = stubs.run(photos, "guided", [20.0, 7.0], [1.5, 3.0])
    want, line = sweep_cli.report("guided", "cnn", 0.1, [20.0, 7.0], [1.5, 3.0], pairs, per_image, has)
    assert list(want) == TODAY and text == json.dumps(want, indent=1)
    assert result["mean_whdr"] == _want_mean(photos, PAIRS).tolist()
    assert capsys.readouterr().out == line + "\n"
    with np.load(str(tmp_path / "sweep.npz")) as saved:
        assert sorted(saved.files) == ["files", "has_judgements", "pairs", "whdr"]
        assert saved["files"].tolist() == photos and np.array_equal(saved["whdr"], per_image)
    # the default is `all`
    os.remove(str(tmp_path / "sweep.json"))
    assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path)) == 0
    with open(str(tmp_path / "sweep.json")) as fh:
        assert fh.read() == text
    # score.py
    argv = ["--inputs", str(tmp_path / "iiw" / "*.png"), "--results", "{dir}/r/{name}", "--out",
            str(tmp_path / "score.json"), "--per_image", str(tmp_path / "score.npz")]
    assert score_cli.main(argv) == 0
    with open(str(tmp_path / "score.json")) as fh:
        assert list(json.load(fh)) == ["coding", "delta", "images", "images_with_judgements", "results",
                                       "source"]
    with np.load(str(tmp_path / "score.npz")) as saved:
        assert sorted(saved.files) == ["files", "has_judgements", "source"]
        assert saved["files"].tolist() == photos
        assert saved["source"].tolist() == [stubs.source_value(f) for f in photos]


@pytest.mark.parametrize("scheme", ["train_val_test", "big_train_mini_val"])
def test_split_test_selects_records_and_averages_what_the_fixture_says(tmp_path, monkeypatch, golden,
                                                                      scheme):
    stubs.install(monkeypatch.setattr)
    _touch(tmp_path / "iiw", golden["stems"])
    for split in ("test", "val"):
        want = [str(tmp_path / "iiw" / (stem + ".png")) for stem in golden[scheme][split]]
        extra = ["--split", split, "--split_scheme", scheme]
        assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path, extra)) == 0
        with open(str(tmp_path / "sweep.json")) as fh:
            result = json.load(fh)
        info = {"name": split, "scheme": scheme, "of": len(golden["stems"]), "images": len(want)}
        assert list(result) == TODAY + ["split"] and result["split"] == info
        assert result["images"] == len(want)
        assert result["images_with_judgements"] == sum(stubs.judged(f) for f in want)
        assert result["mean_whdr"] == _want_mean(want, PAIRS).tolist()
        with np.load(str(tmp_path / "sweep.npz")) as saved:
            assert saved["files"].tolist() == want
            assert saved["whdr"].shape == (4, len(want))
            assert saved["has_judgements"].tolist() == [stubs.judged(f) for f in want]
        # score.py, with a filter
        argv = ["--inputs", str(tmp_path / "iiw" / "*.png"), "--results", "{dir}/r/{name}", "--out",
                str(tmp_path / "score.json"), "--per_image", str(tmp_path / "score.npz"),
                "--filter_type", "guided"] + GRID + extra
        assert score_cli.main(argv) == 0
        with open(str(tmp_path / "score.json")) as fh:
            scored = json.load(fh)
        assert scored["split"] == info and scored["mean_whdr"] == result["mean_whdr"]
        judged = [f for f in want if stubs.judged(f)]
        assert scored["source"]["mean_whdr"] == float(np.mean([stubs.source_value(f) for f in judged]))
        with np.load(str(tmp_path / "score.npz")) as saved:
            assert saved["files"].tolist() == want


@pytest.mark.parametrize("iterations", [1, 3])
def test_report_split_runs_the_best_pair_on_the_other_split(tmp_path, monkeypatch, golden, capsys,
                                                            iterations):
    stubs.install(monkeypatch.setattr)
    _touch(tmp_path / "iiw", golden["stems"])
    val, test = ([str(tmp_path / "iiw" / (stem + ".png")) for stem in golden["train_val_test"][name]]
                 for name in ("val", "test"))
    calls = []
    monkeypatch.setattr(sweep_cli, "run", lambda photos, *a, **kw: (calls.append((list(photos), a[1], a[2])),
                                                                    stubs.run(photos, *a, **kw))[1])
    extra = ["--split", "val", "--report_split", "test", "--iterations", str(iterations)]
    assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path, extra)) == 0
    mean = _want_mean(val, PAIRS, iterations - 1)
    best = PAIRS[int(np.argmin(mean))]
    assert calls == [(val, [20.0, 7.0], [1.5, 3.0]), (test, [best[0]], [best[1]])]
    with open(str(tmp_path / "sweep.json")) as fh:
        result = json.load(fh)
    assert result["split"]["name"] == "val" and result["mean_whdr"] == mean.tolist()
    assert result["best"]["sigma_color"] == best[0] and result["best"]["sigma_spatial"] == best[1]
    report = result["report"]
    keys = ["split", "sigma_color", "sigma_spatial", "mean_whdr", "images", "images_with_judgements"]
    assert list(report) == keys + (["passes"] if iterations > 1 else [])
    assert report["split"] == "test" and (report["sigma_color"], report["sigma_spatial"]) == tuple(best)
    assert report["images"] == len(test) and report["images_with_judgements"] == sum(map(stubs.judged, test))
    assert report["mean_whdr"] == float(_want_mean(test, [best], iterations - 1)[0])
    if iterations > 1:
        assert report["passes"] == [{"pass": k + 1, "mean_whdr": float(_want_mean(test, [best], k)[0])}
                                    for k in range(iterations)]
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("best: ") and lines[1].startswith("test: sigma_color")
    # the grid's files hold the selection split
    with np.load(str(tmp_path / "sweep.npz")) as saved:
        assert saved["files"].tolist() == val


def test_what_the_parsers_refuse(tmp_path, monkeypatch, capsys):
    stubs.install(monkeypatch.setattr)
    _touch(tmp_path / "iiw", ["%d" % i for i in range(1, 24)])

    def refused(tool, argv, words):
        with pytest.raises(SystemExit) as err:
            tool.main(argv)
        assert err.value.code == 2
        message = capsys.readouterr().err
        assert all(word in message for word in words), message
        assert not os.path.exists(str(tmp_path / "sweep.json"))

    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "val", "--split_scheme", "train_test"]),
            ["val", "train_test"])
    refused(score_cli, ["--inputs", "x", "--results", "{name}", "--split", "val", "--split_scheme",
                        "train_test"], ["val", "train_test"])
    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "test", "--report_split", "val",
                                                                "--split_scheme", "train_test"]),
            ["--report_split", "train_test"])
    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "test", "--report_split", "test"]),
            ["--report_split", "test"])
    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--report_split", "test"]),
            ["--report_split", "--split"])
    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "dev"]), ["--split"])
    # the selection split has no judged image: known after its run, refused before the second
    calls = []

    def blind(photos, *a, **kw):
        calls.append(len(photos))
        pairs, per_image, has = stubs.run(photos, *a, **kw)
        return pairs, per_image * 0, has & False

    monkeypatch.setattr(sweep_cli, "run", blind)
    refused(sweep_cli, _sweep_argv(tmp_path / "iiw", tmp_path, ["--split", "val", "--report_split", "test"]),
            ["--report_split", "val", "judgements"])
    assert len(calls) == 1
    assert not os.path.exists(str(tmp_path / "sweep.npz"))


# ---- loader threads ---------------------------------------------------------------------------------------

def test_the_thread_rule():
    assert sharding.io_threads(64) == 16 and sharding.io_threads(64, 1) == 16
    assert sharding.io_threads(64, 8) == 8 and sharding.io_threads(64, 2) == 16
    assert sharding.io_threads(16, 3) == 5 and sharding.io_threads(16, 8) == 2
    assert sharding.io_threads(4, 8) == 1 and sharding.io_threads(1, 1) == 1
    assert sharding.io_threads(4, 8, override=12) == 12 and sharding.io_threads(64, 1, override=40) == 40
    with pytest.raises(ValueError):
        sharding.io_threads(4, 1, override=0)


def test_one_process_keeps_its_threads_and_io_threads_overrides_them(tmp_path, monkeypatch):
    from reflectance_filtering_amd import batch
    stubs.install(monkeypatch.setattr)
    monkeypatch.setattr(batch, "IO_THREADS", batch.IO_THREADS)        # put back after the test
    monkeypatch.setenv("RF_STUB_THREADS_DIR", str(tmp_path))
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(key, raising=False)
    before = batch.IO_THREADS
    _touch(tmp_path / "iiw", ["1", "2", "3"])
    assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path)) == 0
    with open(str(tmp_path / "threads_rank0.json")) as fh:
        assert json.load(fh) == before
    assert sweep_cli.main(_sweep_argv(tmp_path / "iiw", tmp_path, ["--io_threads", "3"])) == 0
    with open(str(tmp_path / "threads_rank0.json")) as fh:
        assert json.load(fh) == 3
    with pytest.raises(SystemExit):
        sweep_cli.build_parser().parse_args(["--inputs", "x"] + GRID + ["--io_threads", "0"])


def test_init_distributed_hands_its_timeout_to_the_group(monkeypatch):
    import datetime
    import torch.distributed as dist
    seen = []
    monkeypatch.setattr(dist, "is_initialized", lambda: False)
    monkeypatch.setattr(dist, "init_process_group", lambda **kw: seen.append(kw))
    for key, text in (("RANK", "1"), ("WORLD_SIZE", "2"), ("LOCAL_RANK", "1")):
        monkeypatch.setenv(key, text)
    monkeypatch.delenv("RF_DIST_BACKEND", raising=False)
    assert sharding.init_distributed() == (1, 2, 1)
    assert sharding.init_distributed(timeout=45) == (1, 2, 1)
    assert seen == [{"backend": "gloo", "rank": 1, "world_size": 2},
                    {"backend": "gloo", "rank": 1, "world_size": 2,
                     "timeout": datetime.timedelta(seconds=45)}]
    assert sweep_cli.parse_args(["--inputs", "x"] + GRID)[1].group_timeout == sweep_cli.GROUP_TIMEOUT
    assert score_cli.parse_args(["--inputs", "x", "--results", "y"]).group_timeout == sweep_cli.GROUP_TIMEOUT
    assert 0 < sweep_cli.GROUP_TIMEOUT < 1800        # finite, and under torch's half hour


# ---- real gloo groups -------------------------------------------------------------------------------------

GROUP_TIMEOUT = 60


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ranks(tool, argv, world, **env_extra):
    """`world` ranks of a tool with the stand-ins installed, each a child process of its own:
    [(return code, stdout, stderr)] in rank order, and the seconds it took."""
    env = dict(os.environ)
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                "RF_DIST_BACKEND", "RF_STUB_FAIL_RANK", "RF_STUB_DIE_RANK", "RF_STUB_THREADS_DIR"):
        env.pop(key, None)
    env.update(env_extra)
    if world > 1:
        env.update(WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, os.path.join(ROOT, "tests", "sweep_stubs.py"), tool] + list(argv)
    cmd += ["--group_timeout", str(GROUP_TIMEOUT)]
    t0 = time.time()
    procs = []
    for rank in range(world):
        rank_env = dict(env, RANK=str(rank), LOCAL_RANK=str(rank)) if world > 1 else env
        procs.append(subprocess.Popen(cmd, env=rank_env, cwd=ROOT, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE))
    done = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=2 * GROUP_TIMEOUT)
            # gloo announces its connections on stdout: not a line of the tool
            own = [line for line in out.decode().splitlines(True) if not line.startswith("[Gloo]")]
            done.append((p.returncode, "".join(own), err.decode()))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return done, time.time() - t0


def _files_of(folder):
    with open(str(folder / "out.json"), "rb") as fh:
        text = fh.read()
    with np.load(str(folder / "out.npz")) as saved:
        return text, {key: saved[key] for key in saved.files}


def _same_files(got, want):
    assert got[0] == want[0]
    assert sorted(got[1]) == sorted(want[1])
    for key, array in want[1].items():
        assert got[1][key].dtype == array.dtype and got[1][key].shape == array.shape, key
        assert np.array_equal(got[1][key], array), key


CASES = {
    "sweep": ("sweep", ["--filter_type", "bilateral"] + GRID),
    "sweep chain on a split": ("sweep", ["--filter_type", "guided", "--iterations", "3", "--split", "train",
                                         "--report_split", "test"] + GRID),
    "score": ("score", ["--results", "{dir}/r/{name}"]),
    "score with a filter": ("score", ["--results", "{dir}/r/{name}", "--filter_type", "guided",
                                      "--iterations", "2", "--split", "test"] + GRID),
}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    folder = tmp_path_factory.mktemp("iiw")
    _touch(folder, ["%d" % i for i in range(1, 18)] + ["10-x"])
    return folder


@pytest.fixture(scope="module")
def one_process(dataset, tmp_path_factory):
    """What one process writes for every case of CASES, computed once."""
    want = {}
    for case, (tool, argv) in CASES.items():
        out = tmp_path_factory.mktemp("one")
        done, _ = _ranks(tool, ["--inputs", str(dataset / "*.png"), "--out", str(out / "out.json"),
                                "--per_image", str(out / "out.npz")] + argv, 1)
        assert done[0][0] == 0, done[0][2][-3000:]
        want[case] = _files_of(out) + (done[0][1],)
    return want


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_files_of_two_and_three_ranks_are_those_of_one_process(dataset, one_process, tmp_path, case,
                                                                  world):
    tool, argv = CASES[case]
    done, _ = _ranks(tool, ["--inputs", str(dataset / "*.png"), "--out", str(tmp_path / "out.json"),
                            "--per_image", str(tmp_path / "out.npz")] + argv, world)
    for rank, (code, out, err) in enumerate(done):
        assert code == 0, (rank, err[-3000:])
    want = one_process[case]
    _same_files(_files_of(tmp_path), want[:2])
    # rank 0 alone prints the result lines and writes; the others say how many photos they had
    assert done[0][1] == want[2] and "photo(s)" not in done[0][2]
    n = len(want[1]["files"])
    for rank in range(1, world):
        lo, hi = sharding.shard_range(n, world, rank)
        assert done[rank][1] == ""
        assert "rank %d: %d photo(s)" % (rank, hi - lo) in done[rank][2]
    assert sorted(os.listdir(str(tmp_path))) == ["out.json", "out.npz"]


def test_three_ranks_on_two_photos(tmp_path):
    folder = tmp_path / "iiw"
    _touch(folder, ["4", "5"])
    assert all(stubs.judged(str(folder / name)) for name in ("4.png", "5.png"))
    outs = {}
    for world in (1, 3):
        out = tmp_path / ("w%d" % world)
        out.mkdir()
        argv = ["--inputs", str(folder / "*.png"), "--out", str(out / "out.json"), "--per_image",
                str(out / "out.npz"), "--filter_type", "guided", "--iterations", "2"] + GRID
        done, _ = _ranks("sweep", argv, world)
        assert [d[0] for d in done] == [0] * world, [d[2][-2000:] for d in done]
        outs[world] = _files_of(out)
        if world == 3:
            assert "rank 1: 1 photo(s)" in done[1][2] and "rank 2: 0 photo(s)" in done[2][2]
    assert outs[1][1]["whdr"].shape == (2, 4, 2)
    _same_files(outs[3], outs[1])


@pytest.mark.parametrize("tool", ["sweep", "score"])
def test_a_rank_that_raises_ends_every_rank_and_nothing_is_written(dataset, tmp_path, tool):
    argv = ["--inputs", str(dataset / "*.png"), "--out", str(tmp_path / "out.json"), "--per_image",
            str(tmp_path / "out.npz")] + CASES[tool][1]
    done, seconds = _ranks(tool, argv, 3, RF_STUB_FAIL_RANK="1")
    assert all(code not in (0, None) for code, _, _ in done), done
    assert seconds < GROUP_TIMEOUT
    photos = sorted(str(dataset / name) for name in os.listdir(str(dataset)))
    lo, _ = sharding.shard_range(len(photos), 3, 1)
    from reflectance_filtering_amd.batch import expand_inputs
    first = expand_inputs([str(dataset / "*.png")])[lo]
    assert "rank 1 failed" in done[0][2] and stubs.FAIL_MESSAGE % first in done[0][2]
    assert "rank 0 failed" not in done[0][2] and "rank 2 failed" not in done[0][2]
    assert done[0][1] == "" and os.listdir(str(tmp_path)) == []


def test_a_rank_that_dies_outright_ends_its_peer_with_an_error(dataset, tmp_path):
    argv = ["--inputs", str(dataset / "*.png"), "--out", str(tmp_path / "out.json"), "--per_image",
            str(tmp_path / "out.npz")] + CASES["sweep"][1]
    done, seconds = _ranks("sweep", argv, 2, RF_STUB_DIE_RANK="1")
    assert done[1][0] == 3 and done[0][0] not in (0, None)
    assert seconds < GROUP_TIMEOUT + 30          # the group's timeout at the latest, not torch's half hour
    assert done[0][1] == "" and os.listdir(str(tmp_path)) == []


def test_under_ranks_the_loader_threads_are_shared_out(dataset, tmp_path):
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    argv = ["--inputs", str(dataset / "*.png"), "--out", str(tmp_path / "out.json")] + CASES["sweep"][1]
    done, _ = _ranks("sweep", argv, 2, RF_STUB_THREADS_DIR=str(tmp_path))
    assert [d[0] for d in done] == [0, 0], [d[2][-2000:] for d in done]
    for rank in range(2):
        with open(str(tmp_path / ("threads_rank%d.json" % rank))) as fh:
            assert json.load(fh) == max(1, min(16, cpus // 2))
    done, _ = _ranks("sweep", argv + ["--io_threads", "5"], 2, RF_STUB_THREADS_DIR=str(tmp_path))
    assert [d[0] for d in done] == [0, 0], [d[2][-2000:] for d in done]
    for rank in range(2):
        with open(str(tmp_path / ("threads_rank%d.json" % rank))) as fh:
            assert json.load(fh) == 5
