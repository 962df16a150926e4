#!/usr/bin/env python3
"""Records the output bits of the per-ray kernels (nvo_weights_pdf, nvo_main_render_loss, nvo_prop_loss,
nvo_prop_loss_pair) on the cases of tests/helpers/per_ray_cases.py: for every (family, case, R) one sha256 over the
inputs and one per output buffer.  Needs the MI355X and a built library.

    python tests/golden/make_golden_per_ray_bits.py tests/golden/per_ray_bits.json --commit $(git rev-parse HEAD)

Re-record only in a change that means to alter these kernels' bits and says so (EXPERIMENTS.md 12.4).
"""
import argparse
import json
import os
import sys

import torch

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
from helpers import per_ray_cases as prc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", help="path of the JSON record to write")
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    record = {"header": {"commit": args.commit, "rocm": torch.version.hip, "torch": torch.__version__,
                         "device": torch.cuda.get_device_name(0)},
              "cases": {}}
    for family, cases in prc.CASES.items():
        for index, case in enumerate(cases):
            for R in prc.RS:
                inp = prc.inputs(family, case, R)
                out = prc.run(family, case, R, inp, device)
                record["cases"][prc.record_key(family, index, R)] = {
                    "inputs": prc.inputs_digest(inp), "outputs": {name: prc.digest(t) for name, t in out.items()}}
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}: {sum(len(c['outputs']) for c in record['cases'].values())} output digests")


if __name__ == "__main__":
    main()
