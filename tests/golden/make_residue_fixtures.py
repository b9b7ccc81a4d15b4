#!/usr/bin/env python3
"""The residue of every atom of the reference's example structures (data, not code), for the set-pair interaction matrix
(include/agbnp_hip.h, agbnp_hip_pair_matrix_*): one line per atom in `particle.id` order, `resid chain resname`.  The order is
that of the trimmed .dms fixtures beside this file: `anum` and `charge` are compared row by row before anything is written.

    python tests/golden/make_residue_fixtures.py <reference checkout>/example
"""
import os
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"trpcage_agbnp1.dms": "residues_trpcage.txt", "1dwc_agbnp1.dms": "residues_1dwc.txt"}


def rows_of(path, columns):
    con = sqlite3.connect(f"file:{path}?mode=ro", uri=True)
    try:
        return con.execute(f"SELECT {columns} FROM particle ORDER BY id").fetchall()
    finally:
        con.close()


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    for dms, out in FILES.items():
        rows = rows_of(os.path.join(sys.argv[1], dms), "id, anum, charge, resid, chain, resname")
        assert [r[:3] for r in rows] == rows_of(os.path.join(HERE, dms), "id, anum, charge"), f"{dms}: another atom order"
        assert all(str(field).strip() and len(str(field).split()) == 1 for r in rows for field in r[3:]), f"{dms}: an empty label"
        with open(os.path.join(HERE, out), "w") as f:
            f.writelines(f"{resid} {chain} {resname}\n" for (_, _, _, resid, chain, resname) in rows)
        print(out, len(rows), "atoms,", len({r[3:] for r in rows}), "residues")
