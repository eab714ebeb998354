"""Record tests/golden/patch_layout_digests.json: the digests of tests/patch_layout_cases.py, computed on the GPU with the
library that SVO_LIB names.  That library must be built from the commit whose layout the fixture pins (a checkout of it in
a scratch directory outside the repository), never from the code under test: tests/test_gpu_patch_layout.py then
recomputes the digests with the tree's own library.
usage: SVO_LIB=/path/to/pinned/libsvo_rt.so python tools/record_patch_layout_digests.py COMMIT [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("SVO_LIB"), "SVO_LIB must name the pinned commit's library"
    import patch_layout_cases as plc
    import raytracing_test_amd as rt

    assert os.path.samefile(rt.LIB_PATH, os.environ["SVO_LIB"])
    digests = dict(plc.all_cases(rt))
    out = {"recorded_from_commit": sys.argv[1], "library_build_id": rt.build_id(), "digests": digests}
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "patch_layout_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests from %s -> %s" % (len(digests), sys.argv[1], path))


if __name__ == "__main__":
    main()
