"""CPU suite: the two classes of tests/test_gpu_capture_contract.py against the header - every entry of
include/reflectance_filtering.h that takes a `stream` is capturable or refusing and not both, every case
is run by exactly one of the two parametrised tests, the refusing class is the synchronising class plus the
two raw-weight CNN entries, and the header text of every refusing entry says that it is refused while its
stream is being captured.  No GPU, no library (one test builds the module's own cases on the host)."""
import os
import re

from tests import test_gpu_capture_contract as cc
from tests import test_gpu_stream_contract as sc
from tests.test_stream_cases import _entries_with_a_stream, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(test):
    """The ids a parametrised test runs, from its own mark."""
    marks = [m for m in test.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "name"
    return list(marks[0].args[1])


def test_every_entry_that_takes_a_stream_is_in_exactly_one_class():
    names = _entries_with_a_stream(_header())
    assert len(names) >= 21, names
    assert len(set(cc.REFUSING)) == len(cc.REFUSING) and len(set(cc.CAPTURABLE)) == len(cc.CAPTURABLE)
    assert not set(cc.REFUSING) & set(cc.CAPTURABLE), set(cc.REFUSING) & set(cc.CAPTURABLE)
    assert sorted(cc.REFUSING + cc.CAPTURABLE) == names, set(cc.REFUSING + cc.CAPTURABLE) ^ set(names)


def test_the_refusing_class_is_the_synchronising_class_and_the_raw_weight_cnn_entries():
    assert set(sc.SYNCHRONISING) <= set(cc.REFUSING)
    assert set(cc.REFUSING) - set(sc.SYNCHRONISING) == {"rf_cnn_reflectance_u8", "rf_cnn_reflectance_f32"}


def test_every_case_is_run_by_exactly_one_of_the_two_tests():
    captured = _ids(cc.test_capturable_case_is_captured_and_replays)
    refused = _ids(cc.test_refusing_case_is_refused_and_leaves_the_capture_alone)
    assert len(set(captured)) == len(captured) and len(set(refused)) == len(refused)
    assert not set(captured) & set(refused), set(captured) & set(refused)
    cases = cc.all_cases()
    assert set(sc.CASES) < set(cases) and set(cases) - set(sc.CASES) == set(cc.EXTRA)
    assert sorted(captured + refused) == sorted(cases), set(captured + refused) ^ set(cases)
    for name in captured:
        assert not set(cases[name][0]) & set(cc.REFUSING), name
        assert set(cases[name][0]) <= set(cc.CAPTURABLE), name
    for name in refused:
        assert set(cases[name][0]) & set(cc.REFUSING), name
    # every entry of either class is reached, the lifecycle test runs every case of the shared list, the cold
    # case and the three fallback refusals are there
    assert set(e for name in captured for e in cases[name][0]) == set(cc.CAPTURABLE)
    assert set(e for name in refused for e in cases[name][0]) == set(cc.REFUSING)
    assert _ids(cc.test_entry_across_shutdown_and_release_scratch) == sorted(sc.CASES)
    assert set(cc.COLD) <= set(captured) and all(cases[name][2].get("cold") for name in cc.COLD)
    assert len(set(cc.EXTRA) & set(refused)) == 3
    assert set(cc.CROSSING) <= set(sc.CASES) and len(set(cc.CROSSING)) == 5


def test_the_cases_of_the_capture_module_build_on_the_host(built):
    """The cases the module adds to the shared list: the entries they name, a decoy for every value input, the
    fallback routes (asserted by the builders from the library's own plans), and a sigma_color of the cold case
    that no other test module names."""
    import numpy as np
    import torch

    import reflectance_filtering_amd as rf
    from oracle import c_oracle as co
    from tests import abi_cases as C
    env = (rf, co, torch)
    for name in sorted(cc.EXTRA):
        entries, build, opts = cc.EXTRA[name]
        case = build(env)
        assert case.entries == entries, name
        assert case.sync == any(e in sc.SYNCHRONISING for e in entries), name
        for b in case.bufs:
            if b.data is not None and b.name not in C.INDEX_LIKE:
                assert b.decoy is not None and not np.array_equal(b.decoy, b.data), (name, b.name)
    here = os.path.join(ROOT, "tests")
    for fname in sorted(os.listdir(here)):
        if fname.endswith(".py") and fname not in ("test_gpu_capture_contract.py", os.path.basename(__file__)):
            with open(os.path.join(here, fname)) as fh:
                assert "19.4375" not in fh.read(), fname


def test_the_header_text_of_every_refusing_entry_speaks_of_the_refusal():
    """The comment block in front of a refusing entry's declaration says that the call is refused while its
    stream is being captured; where the block serves several entries, the sentence names this one."""
    text = _header()
    names = _entries_with_a_stream(text)
    blocks = {}
    for name in names:
        at = re.search(r"^int %s\(" % name, text, flags=re.M).start()
        start = text.rfind("\n/*", 0, at)
        blocks[name] = (start, re.sub(r"\s*\n\s*\*?\s*", " ", text[start:at]))
    for name in cc.REFUSING:
        start, comment = blocks[name]
        shared = [other for other in names if other != name and blocks[other][0] == start]
        assert "captur" in comment, name
        says = r"refus[^.]*captur|captur[^.]*refus"
        if shared:
            says = r"\b%s\b[^.]*(?:%s)" % (name, says)
        assert re.search(says, comment), (name, shared)
    # ... and the preamble states the classes and names the module
    graphs = text[text.index(" * Graphs ("):text.index(" * Sizes (")]
    assert "tests/test_gpu_capture_contract.py" in graphs and "rf_shutdown" in graphs
    listed = set(re.findall(r"\brf_[a-z0-9_]+", graphs))
    assert set(cc.CAPTURABLE) - {"rf_cnn_reflectance_packed_u8", "rf_cnn_reflectance_packed_f32"} <= listed
    assert "rf_cnn_reflectance_packed" in listed
    assert {"rf_cnn_reflectance_u8", "rf_cnn_reflectance_f32"} <= listed and "SYNCHRONISES THE STREAM" in graphs
