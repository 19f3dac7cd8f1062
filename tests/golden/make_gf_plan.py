#!/usr/bin/env python
"""Record tests/golden/gf_plan_parent.json: what the guided filter's host code planned and refused at
the commit BEFORE rf_gf.hip was split by role (tests/test_gf_plan_pinned.py holds every later commit to it).

    git worktree add /tmp/gf_parent 92f4b3e && make -C /tmp/gf_parent/reflectance_filtering_amd/csrc -j8
    python tests/golden/make_gf_plan.py --package-root /tmp/gf_parent

--package-root names the checkout whose reflectance_filtering_amd package (and librf_hip.so) answers;
the table of calls is this checkout's tests/gf_plan_cases.py.  No device is needed or used.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PARENT = "92f4b3e"      # "Score sRGB-coded and unfiltered stored results: WHDR value tables"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", required=True, help="checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "gf_plan_parent.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from reflectance_filtering_amd import _ffi
    assert os.path.abspath(_ffi.__file__).startswith(os.path.abspath(args.package_root)), _ffi.__file__
    import importlib.util   # (by path: the parent checkout has a `tests` package of its own)
    spec = importlib.util.spec_from_file_location("gf_plan_cases", os.path.join(REPO, "tests", "gf_plan_cases.py"))
    gf_plan_cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gf_plan_cases)
    data = {"parent": PARENT}
    data.update(gf_plan_cases.record(_ffi))
    with open(args.out, "w") as f:
        f.write("{\n")
        keys = list(data)
        for k in keys:
            v = data[k]
            end = ",\n" if k != keys[-1] else "\n"
            if isinstance(v, list):     # one row per line
                f.write(' "%s": [\n' % k + ",\n".join("  " + json.dumps(row) for row in v) + "\n ]" + end)
            else:
                f.write(' "%s": %s' % (k, json.dumps(v)) + end)
        f.write("}\n")
    print("wrote %s: %s" % (args.out, ", ".join("%s %d" % (k, len(v)) for k, v in data.items() if isinstance(v, list))))


if __name__ == "__main__":
    main()
