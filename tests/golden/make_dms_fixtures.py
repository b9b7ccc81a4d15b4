#!/usr/bin/env python3
"""Trimmed copies of the reference's example structures (data, not code) for tests/test_host_api.py's .dms loader test:
the two tables and the columns load_dms() reads -- particle(id, anum, x, y, z, charge) and agbnp2(id, radius, igamma) --
row for row and value for value, in the tables' own order.  What a Desmond .dms holds beyond that (force-field terms,
names, velocities) is left out, so the fixtures stay small and the test needs nothing outside the repository.

    python tests/golden/make_dms_fixtures.py <reference checkout>/example
"""
import os
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ("trpcage_agbnp1.dms", "1dwc_agbnp1.dms")


def trim(src, dst):
    con = sqlite3.connect(f"file:{src}?mode=ro", uri=True)
    try:
        particles = con.execute("SELECT id, anum, x, y, z, charge FROM particle ORDER BY rowid").fetchall()
        agbnp2 = con.execute("SELECT id, radius, igamma FROM agbnp2 ORDER BY rowid").fetchall()
    finally:
        con.close()
    if os.path.exists(dst):
        os.remove(dst)
    out = sqlite3.connect(dst)
    with out:
        out.execute("CREATE TABLE particle (id integer primary key, anum integer, x float, y float, z float, charge float)")
        out.execute("CREATE TABLE agbnp2 (id INTEGER NOT NULL REFERENCES particle, radius FLOAT, igamma FLOAT)")
        out.executemany("INSERT INTO particle VALUES (?, ?, ?, ?, ?, ?)", particles)
        out.executemany("INSERT INTO agbnp2 VALUES (?, ?, ?)", agbnp2)
    out.execute("VACUUM")
    out.close()
    return len(particles), len(agbnp2)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    for name in FILES:
        print(name, trim(os.path.join(sys.argv[1], name), os.path.join(HERE, name)))
