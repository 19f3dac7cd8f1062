"""GPU suite: the sweep and the score at dataset scale (sweep.run_sharded, --split / --report_split).

What the merge of the ranks' results stands on is tested first, in one process: the columns of
sweep.run(photos) equal those of sweep.run(photos[lo:hi]) exactly, for the slices two and three ranks
take - a photo's WHDR does not depend on what else is in its pack.  Then two ranks on one device, as
child processes under RANK / WORLD_SIZE / LOCAL_RANK, against one process: the JSON byte for byte,
the npz array for array.  Every comparison is exact equality; there is no tolerance anywhere.

Seven photos of 48x64, 60x80 and 64x48, ordered so that every slice boundary of the 2-way (4 | 3) and
the 3-way cut (3 | 2 | 2) falls between two shapes; about 20 judgements each, photo 2 has none; stored
sources of which 0, 2, 3 and 6 have three equal channels.  The grid holds the pairs c20 s22 and c7 s9.
"""
import json
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (env is a fixture)
from tests.test_gpu_jbf_points import _comparisons, _write_iiw_json

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(48, 64), (60, 80), (64, 48), (48, 64), (60, 80), (64, 48), (60, 80)]
NO_JUDGEMENTS = 2
GREY_SOURCES = (0, 2, 3, 6)
PAIR = {"bilateral": ([20.0], [22.0]), "guided": ([7.0], [9.0])}
GRID = ["--sigma_color", "20,7", "--sigma_spatial", "22,9"]
CHILD_SECONDS = 150         # the time limit of one rank
GROUP_TIMEOUT = 60


def _write_photos(folder, shapes, seed, no_judgements, grey_sources):
    """Photos `<k>.png` with judgement files beside them, a stored source under src/ and a guidance
    image under flat/ for each: the photo names."""
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from tests import synth
    rng = np.random.default_rng(seed)
    for d in ("src", "flat"):
        (folder / d).mkdir()
    names = []
    for i, (h, w) in enumerate(shapes):
        name = str(folder / ("%02d.png" % i))
        iu.imwrite(name, synth.scene_u8(h, w, seed + i))
        iu.imwrite(str(folder / "flat" / ("%02d.png" % i)), synth.flat_guide_u8(h, w, seed + 100 + i, cells=6))
        source = (synth.reflectance_like_u8 if i in grey_sources else synth.scene_u8)(h, w, seed + 200 + i)
        iu.imwrite(str(folder / "src" / ("%02d.png" % i)), source)
        _write_iiw_json(sweep_cli.judgements_for(name),
                        _comparisons(h, w, rng, 0 if i == no_judgements else 20), h, w)
        names.append(name)
    return names


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    folder = tmp_path_factory.mktemp("iiw7")
    return folder, _write_photos(folder, SHAPES, 7300, NO_JUDGEMENTS, GREY_SOURCES)


# ---- slice independence, in one process -------------------------------------------------------------------

SLICE_CASES = {
    "prediction": {},
    "prediction guided by the photo": {"guidance": "image"},
    "prediction twice": {"iterations": 2},
    "stored": {"src_files": "{dir}/src/{name}"},
    "stored twice guided by files": {"src_files": "{dir}/src/{name}", "guidance_files": "{dir}/flat/{name}",
                                     "iterations": 2},
}


@pytest.mark.parametrize("case", sorted(SLICE_CASES))
@pytest.mark.parametrize("ftype", ["bilateral", "guided"])
def test_the_columns_of_a_slice_are_those_of_the_whole_list(env, dataset, ftype, case):
    from reflectance_filtering_amd import sharding
    from reflectance_filtering_amd import sweep as sweep_cli
    _, photos = dataset
    kwargs = SLICE_CASES[case]
    sigma_color, sigma_spatial = PAIR[ftype]
    pairs, whole, has = sweep_cli.run(photos, ftype, sigma_color, sigma_spatial, **kwargs)
    assert whole.shape[-1] == len(photos) and whole.dtype == np.float64
    assert has.tolist() == [i != NO_JUDGEMENTS for i in range(len(photos))]
    assert np.any(whole > 0) and np.all(whole[..., NO_JUDGEMENTS] == 0)
    for world in (2, 3):
        cuts = [sharding.shard_range(len(photos), world, rank) for rank in range(world)]
        for lo, hi in cuts[:-1]:
            assert SHAPES[hi - 1] != SHAPES[hi], "a slice boundary between two shapes"
        for lo, hi in cuts:
            _, part, part_has = sweep_cli.run(photos[lo:hi], ftype, sigma_color, sigma_spatial, **kwargs)
            for i in range(lo, hi):
                print("%s %s, %d ranks, photo %d: slice %s whole %s"
                      % (ftype, case, world, i, part[..., i - lo].ravel().tolist(), whole[..., i].ravel().tolist()))
            assert np.array_equal(part, whole[..., lo:hi]), (world, lo, hi)
            assert part_has.tolist() == has[lo:hi].tolist()


# ---- two ranks on one device against one process ----------------------------------------------------------

def _clean_env(**extra):
    env_ = dict(os.environ)
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                "RF_DIST_BACKEND"):
        env_.pop(key, None)
    env_.update(extra)
    return env_


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ranks(tool, argv, world, logs):
    """`world` ranks of a tool, each a child process under a time limit of its own, all at once (with
    this process at most three hold the device).  The first rank found to have ended non-zero fails the
    test and the others are killed; nothing is started again.  Returns the ranks' (stdout, stderr)."""
    port = _free_port()
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-m",
           "reflectance_filtering_amd." + tool] + list(argv) + ["--group_timeout", str(GROUP_TIMEOUT)]
    procs, files = [], []
    for rank in range(world):
        extra = {} if world == 1 else dict(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                                           LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                           MASTER_PORT=str(port))
        out = open(str(logs / ("w%d_rank%d.out" % (world, rank))), "w+")
        err = open(str(logs / ("w%d_rank%d.err" % (world, rank))), "w+")
        files.append((out, err))
        procs.append(subprocess.Popen(cmd, cwd=ROOT, env=_clean_env(**extra), stdout=out, stderr=err,
                                      start_new_session=True))      # killed with what it started
    texts = []
    try:
        for rank, p in enumerate(procs):
            code = p.wait(timeout=CHILD_SECONDS + 30)
            for fh in files[rank]:
                fh.seek(0)
            texts.append((files[rank][0].read(), files[rank][1].read()))
            assert code == 0, "rank %d of %d ended with %d: %s" % (rank, world, code, texts[-1][1][-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
        for pair in files:
            for fh in pair:
                fh.close()
    return texts


def _files_of(folder):
    with open(str(folder / "out.json"), "rb") as fh:
        text = fh.read()
    with np.load(str(folder / "out.npz")) as saved:
        return text, {key: saved[key] for key in saved.files}


RANK_CASES = {
    "sweep bilateral": ("sweep", ["--filter_type", "bilateral"] + GRID),
    "sweep guided": ("sweep", ["--filter_type", "guided"] + GRID),
    "sweep stored twice": ("sweep", ["--filter_type", "guided", "--src_files", "{dir}/src/{name}",
                                     "--iterations", "2"] + GRID),
    "score with a filter": ("score", ["--results", "{dir}/src/{name}", "--coding", "srgb",
                                      "--filter_type", "bilateral"] + GRID),
}


@pytest.mark.parametrize("case", sorted(RANK_CASES))
def test_two_ranks_on_one_device_write_the_files_of_one_process(env, dataset, tmp_path, case):
    folder, photos = dataset
    tool, argv = RANK_CASES[case]
    written = {}
    for world in (1, 2):
        out = tmp_path / ("w%d" % world)
        out.mkdir()
        texts = _ranks(tool, ["--inputs", str(folder / "*.png"), "--out", str(out / "out.json"),
                              "--per_image", str(out / "out.npz")] + argv, world, tmp_path)
        written[world] = _files_of(out)
        lines = [ln for ln in texts[0][0].splitlines() if not ln.startswith("[Gloo]")]
        assert lines and lines[-1].startswith("best: sigma_color")
        if world == 2:
            assert "rank 1: 3 photo(s)" in texts[1][1]
            assert [ln for ln in texts[1][0].splitlines() if not ln.startswith("[Gloo]")] == []
    (one_json, one), (two_json, two) = written[1], written[2]
    print(one_json.decode())
    result = json.loads(one_json.decode())
    assert result["images"] == 7 and result["images_with_judgements"] == 6 and "split" not in result
    assert one["files"].tolist() == photos and one["whdr"].shape[-2:] == (4, 7)
    assert np.any(one["whdr"] > 0) and one["has_judgements"].tolist() == [i != NO_JUDGEMENTS for i in range(7)]
    assert two_json == one_json
    assert sorted(two) == sorted(one)
    for key, array in one.items():
        assert two[key].dtype == array.dtype and two[key].shape == array.shape, key
        assert np.array_equal(two[key], array), key


# ---- the paper's protocol ---------------------------------------------------------------------------------

def test_split_val_report_split_test_equals_the_two_runs_by_hand(env, tmp_path, capsys):
    from reflectance_filtering_amd import sweep as sweep_cli
    shapes = [(12 + (i % 3) * 3, 16 + (i % 4) * 2) for i in range(20)]
    photos = _write_photos(tmp_path, shapes, 7600, 5, ())
    # the stems 00..19 are in order: val holds positions 6 and 16, test 0, 5, 10 and 15
    val, test = [photos[k] for k in (6, 16)], [photos[k] for k in (0, 5, 10, 15)]
    out, npz = str(tmp_path / "out.json"), str(tmp_path / "out.npz")
    argv = ["--inputs", str(tmp_path / "*.png"), "--filter_type", "bilateral", "--sigma_color", "20,7",
            "--sigma_spatial", "2.5,4", "--split", "val", "--report_split", "test", "--out", out,
            "--per_image", npz]
    assert sweep_cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    with open(out) as fh:
        result = json.load(fh)
    pairs, chosen_on, has = sweep_cli.run(val, "bilateral", [20.0, 7.0], [2.5, 4.0])
    mean = chosen_on[:, has].mean(axis=1)
    best = int(np.argmin(mean))
    print("val means", mean.tolist(), "best", pairs[best].tolist())
    assert len(set(mean.tolist())) > 1, "the grid has to tell its pairs apart"
    assert result["split"] == {"name": "val", "scheme": "train_val_test", "of": 20, "images": 2}
    assert result["mean_whdr"] == mean.tolist()
    assert result["best"] == {"sigma_color": pairs[best, 0], "sigma_spatial": pairs[best, 1],
                              "mean_whdr": mean[best]}
    _, held_out, test_has = sweep_cli.run(test, "bilateral", [pairs[best, 0]], [pairs[best, 1]])
    assert test_has.tolist() == [True, False, True, True]
    assert result["report"] == {"split": "test", "sigma_color": pairs[best, 0],
                                "sigma_spatial": pairs[best, 1],
                                "mean_whdr": float(held_out[:, test_has].mean(axis=1)[0]), "images": 4,
                                "images_with_judgements": 3}
    assert len(lines) == 2 and lines[1].startswith("test: sigma_color")
    with np.load(npz) as saved:
        assert saved["files"].tolist() == val and np.array_equal(saved["whdr"], chosen_on)
