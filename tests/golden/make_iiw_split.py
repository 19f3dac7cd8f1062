#!/usr/bin/env python
"""Record tests/golden/iiw_split.json: the lists the reference's three split functions return for one
list of stems (tests/test_sweep_dataset.py holds whdr.iiw_split to them, list for list).

    python tests/golden/make_iiw_split.py --reference <checkout of the reference>

The functions - narihiraSplitIntoTwoLists, narihiraSplitIntoThreeLists, splitIntoBigTrainMiniVal of
training/createNumpyArrayWithComparisonsForIIW.py - are taken out of the reference's file with `ast`
and run alone: the module itself imports cv2 and reads a data folder when it is run.  They get the
stems sorted as the reference's main part sorts its file names (list.sort(), plain string order).

The stems, written into the fixture in a shuffled order: the ids 1..117 as IIW names its photos
(so `9`, `10` and `100` are among them and string order is not numeric order), `10-x` (as a file
name `10-x.png` sorts before `10.png`, as a stem after `10`), `100_b`, `Zebra` (upper case sorts before
lower case and after the digits) and one non-ASCII stem: 121 in all, so that position 106 - the second
`k % 100 == 6` - exists.
"""
import argparse
import ast
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join("training", "createNumpyArrayWithComparisonsForIIW.py")
FUNCTIONS = {"train_test": ("narihiraSplitIntoTwoLists", ("train", "test")),
             "train_val_test": ("narihiraSplitIntoThreeLists", ("train", "val", "test")),
             "big_train_mini_val": ("splitIntoBigTrainMiniVal", ("train", "val", "test"))}


def stems():
    names = [str(i) for i in range(1, 118)] + ["10-x", "100_b", "Zebra", u"café-7"]
    random.Random(689).shuffle(names)
    return names


def reference_functions(path):
    """The three functions, compiled from their own source lines alone."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    wanted = {name for name, _ in FUNCTIONS.values()}
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in wanted]
    assert {node.name for node in picked} == wanted, "not all split functions found in %s" % path
    scope = {}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), scope)
    return scope


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "iiw_split.json"))
    args = ap.parse_args()
    scope = reference_functions(os.path.join(args.reference, SOURCE))
    data = {"stems": stems()}
    file_names = list(data["stems"])
    file_names.sort()
    for scheme, (function, parts) in FUNCTIONS.items():
        lists = scope[function](list(file_names))
        assert len(lists) == len(parts)
        data[scheme] = dict(zip(parts, lists))
    with open(args.out, "w") as fh:
        json.dump(data, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d stems" % (args.out, len(data["stems"])))


if __name__ == "__main__":
    main()
