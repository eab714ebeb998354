"""Record tests/golden/linearised_digests.json: the digests of tests/linearise_cases.py, computed with the library that
SVO_LIB names.  That library must be built from the commit whose layout the fixture pins (a checkout of it in a scratch
directory outside the repository), never from the code under test: tests/test_linearise_host.py then recomputes the
digests with the tree's own library.
usage: SVO_LIB=/path/to/pinned/libsvo_rt.so python tools/record_linearised_digests.py COMMIT"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("SVO_LIB"), "SVO_LIB must name the pinned commit's library"
    import linearise_cases as lc
    import raytracing_test_amd as rt
    from oracle import oracle as O

    O.build()
    assert os.path.samefile(rt.LIB_PATH, os.environ["SVO_LIB"])
    digests = dict(lc.static_cases(rt))
    for levels in lc.LEVELS:
        digests.update(lc.script_cases(rt, O, levels))
    out = {"recorded_from_commit": sys.argv[1], "library_build_id": rt.build_id(), "digests": digests}
    path = os.path.join(ROOT, "tests", "golden", "linearised_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests from %s -> %s" % (len(digests), sys.argv[1], path))


if __name__ == "__main__":
    main()
