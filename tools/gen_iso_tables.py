#!/usr/bin/env python3
"""Writes nerf-vo_amd/csrc/iso_tables.h, the case tables of the HIP iso-surface extractor (csrc/iso.hip), from the tables
of nerf_vo_amd/meshing.py.  Run it after changing _CORNERS, _TETS, _TABLE or the winding rule there:

    python tools/gen_iso_tables.py          # rewrite the header
    python tools/gen_iso_tables.py --check  # exit status 1 if the committed header is out of date
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "nerf-vo_amd", "csrc", "iso_tables.h")

if __name__ == "__main__":
    from nerf_vo_amd.meshing import iso_tables_header

    text = iso_tables_header()
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(HEADER) and open(HEADER).read() == text else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print("wrote", HEADER)
