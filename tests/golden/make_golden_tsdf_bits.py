#!/usr/bin/env python3
"""Records the output bits of the TSDF fusion kernels and the edge-owned extractors (nvo_tsdf_integrate,
nvo_tsdf_blocks_touch / _integrate / _iso_count / _iso_emit, nvo_iso_count / _emit) on the cases of
tests/helpers/tsdf_bits_cases.py: one sha256 over the inputs and one per output tensor, and next to the record
(<out without .json>_inputs.npz) the frames themselves.  Needs the MI355X and a built library.

    python tests/golden/make_golden_tsdf_bits.py tests/golden/tsdf_bits.json --commit $(git rev-parse HEAD)

Re-record only in a change that means to alter the fusion rule's or the extractor's bits and says so.
"""
import argparse
import json
import os
import sys

import torch

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
from helpers import tsdf_bits_cases as tbc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", help="path of the JSON record to write")
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    inputs_path = os.path.splitext(args.out)[0] + "_inputs.npz"
    tbc.save_inputs(tbc.scene_inputs(), inputs_path)
    inp = tbc.inputs(inputs_path)
    out = tbc.run(inp, device)
    record = {"header": {"commit": args.commit, "rocm": torch.version.hip, "torch": torch.__version__,
                         "device": torch.cuda.get_device_name(0)},
              "inputs": tbc.inputs_digest(inp),
              "cases": {case: {name: tbc.digest(t) for name, t in tensors.items()} for case, tensors in out.items()}}
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(f"wrote {inputs_path} and {args.out}: {sum(len(c) for c in record['cases'].values())} output digests")


if __name__ == "__main__":
    main()
