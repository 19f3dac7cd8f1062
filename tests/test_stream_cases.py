"""CPU suite: the case list of tests/test_gpu_stream_contract.py against the header - every entry of
include/reflectance_filtering.h that takes a `stream` is run by that module, and the entries it holds to
"one synchronisation of the stream" are exactly those whose header text says so.  No GPU, no library."""
import os
import re

from tests import test_gpu_stream_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "reflectance_filtering.h")) as fh:
        return fh.read()


def _entries_with_a_stream(text):
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(name for name, args in re.findall(r"\b(rf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)
                  if re.search(r"\bvoid\s*\*\s*stream\b", args))


def test_every_entry_that_takes_a_stream_is_in_the_stream_contract_module():
    names = _entries_with_a_stream(_header())
    assert len(names) >= 21 and "rf_jbf_u8" in names and "rf_cnn_pack_weights" in names, names
    assert sc.covered_entries() == names, sorted(set(sc.covered_entries()) ^ set(names))
    for entries, build, opts in sc.CASES.values():
        assert entries and callable(build)
        assert set(opts) <= {"two_wg", "cold", "form"}, opts


def test_every_case_builds_on_the_host_and_every_value_input_has_a_decoy(built):
    """Building a case needs the library's size queries and plans only.  Checked for every case: the
    entries and the class it is listed under, a decoy that differs from the true data for every input that
    is not index-like (a GPU run that read a missing decoy's place would read the arena's fill), the route
    the list names (two workgroups per CU, the kernel form of rf_jbf_f32)."""
    import numpy as np
    import torch

    import reflectance_filtering_amd as rf
    from oracle import c_oracle as co
    from tests import abi_cases as C
    env = (rf, co, torch)
    for name in sorted(sc.CASES):
        entries, build, opts = sc.CASES[name]
        case = build(env)
        assert case.entries == entries, name
        assert case.sync == any(e in sc.SYNCHRONISING for e in entries), name
        for b in case.bufs:
            if b.data is None:
                assert b.role in ("out", "ws"), (name, b.name)
            elif b.decoy is None:
                assert b.name in C.INDEX_LIKE, (name, b.name)
            else:
                assert b.name not in C.INDEX_LIKE and not np.array_equal(b.decoy, b.data), (name, b.name)
                assert np.isfinite(b.decoy.astype(np.float64)).all(), (name, b.name)
        if opts.get("two_wg"):
            assert case.two_wg, name
        if "form" in opts:
            joint = [b for b in case.bufs if b.name == "joint"][0]
            assert sc._jbf_f32_form(joint.data, *sc.F32_FORMS[opts["form"]]) == opts["form"], name
            # the decoy keeps the joint's value range, image by image: a stale read stays inside the table
            for true, decoy in zip(joint.data, joint.decoy):
                assert true.min() == decoy.min() and true.max() == decoy.max(), name


def test_the_synchronising_class_is_the_header_text():
    """An entry is in the synchronising class exactly if the comment in front of its declaration says, in
    capitals, that it synchronises the stream."""
    text = _header()
    names = _entries_with_a_stream(text)
    assert set(sc.SYNCHRONISING) <= set(names)
    says = set()
    for name in names:
        at = re.search(r"^int %s\(" % name, text, flags=re.M).start()
        comment = text[text.rfind("\n/*", 0, at):at]      # (the block comment, not a #define's remark)
        for m in re.finditer(r"SYNCHRONISES\s+THE\s+STREAM", comment):
            # (a comment that serves two entries gives each a paragraph headed "rf_name:")
            headed = re.findall(r"^\s*\*\s+(rf_[a-z0-9_]+):", comment[:m.start()], flags=re.M)
            if headed and headed[-1] != name and headed[-1] in names:
                continue
            says.add(name)
    assert says == set(sc.SYNCHRONISING), says ^ set(sc.SYNCHRONISING)
