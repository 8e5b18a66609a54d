"""Records the host layer's call log for every case of tests/conv_host_cases.py -> tests/golden/conv_host_parent.json.

Run once, without a GPU, in a checkout of the commit BEFORE the host layer was reworked (with the library built, and only
tests/conv_host_log.py, tests/conv_host_cases.py and this file added to it):

    python tests/golden/make_conv_host_golden.py

The file holds the commit it ran at and {case name: sha256 of the case's canonical log}.

    python tests/golden/make_conv_host_golden.py --dump "layer dec.1.1 2x48x64 mma0 tile0x0"

prints one case's canonical log, with the planned route of every conv launch and every record's `executed` beside it, so that a mismatch
can be diffed between two checkouts."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "unsupervised-pseuso-lidar_amd"), REPO]

import conv_host_cases as C  # noqa: E402


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        sys.stdout.write(C.dump(sys.argv[2], C.all_cases()[sys.argv[2]]))
        return
    git = lambda *a: subprocess.check_output(("git", "-C", REPO) + a, text=True).strip()
    if git("status", "--porcelain", "--untracked-files=no"):
        raise SystemExit("the checkout differs from its commit: the golden is recorded at a commit")
    out = {"commit": git("rev-parse", "--short", "HEAD"), "cases": C.hashes()}
    path = os.path.join(HERE, "conv_host_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases at %s" % (path, len(out["cases"]), out["commit"]))


if __name__ == "__main__":
    main()
