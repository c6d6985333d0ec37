#!/usr/bin/env python3
"""The point-triangle routines of csrc/mesh_distance_device.h on the host against the fp64 restatement, per row of the
single-face grid of tests/thin_faces.py: worst error and number of queries over the 5e-7 m bar (tests/test_thin_faces.py asserts
the same for the working tree).  With --rev the header is taken from that git revision (a copy in a temporary directory), which
shows what the tests would have said of an earlier header.  Needs hipcc; no GPU.  Prints a markdown table."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", help="git revision whose mesh_distance_device.h is used (default: the working tree's)")
    a = ap.parse_args()
    import test_thin_faces as T
    import thin_faces as TF
    with tempfile.TemporaryDirectory() as tmp:
        hdr = None
        if a.rev:
            hdr = os.path.join(tmp, "hdr")
            os.mkdir(hdr)
            text = subprocess.run(["git", "-C", ROOT, "show", f"{a.rev}:hands_amd/csrc/mesh_distance_device.h"], check=True,
                                  capture_output=True).stdout
            with open(os.path.join(hdr, "mesh_distance_device.h"), "wb") as fh:
                fh.write(text)
        table = T.row_table(T.build_host(tmp, hdr), tmp)
    print(f"header: {a.rev or 'working tree'}; bar {T.BAR:g} m\n")
    print("| shape | L (m) | height / L | centre | faces | queries | worst error (m) | over the bar |")
    print("|---|---|---|---|---|---|---|---|")
    for row, ((shape, L, ratio, centre), (worst, over, n)) in enumerate(zip(TF.ROWS, table)):
        print(f"| {shape} | {L:g} | {ratio:g} | {'z = 0.5' if centre else 'origin'} | {6 * TF.n_orient(row)} | {n} | {worst:.2e} | {over} |")
    thin = [t[1] for spec, t in zip(TF.ROWS, table) if spec[2] <= 1e-4]
    print(f"\nrows with height / L <= 1e-4: {len(thin)}, fewest queries over the bar among them: {min(thin)}; "
          f"rows over the bar in all: {sum(t[1] > 0 for t in table)} of {len(table)}")


if __name__ == "__main__":
    main()
