#!/usr/bin/env python3
"""What pair-matrix groups and the set-pair matrix of a binding energy cost (include/agbnp_hip.h: agbnp_hip_pair_matrix_group,
agbnp_hip_binding_pair_matrix_device), beside what a caller could write before they existed, and that adding
them has left the full evaluation alone.

(a) One child process per group size: microseconds per pair_matrix_group() call over R trpcage contexts with the residue
    partition, and per round of the same members' R pair_matrix_device() calls back to back, in the same process.
(b) One child process per system: microseconds per BindingEnergy.pair_matrix_device() call, and per call of the BASELINE in the
    same process -- three contexts (complex, receptor, ligand) with the partition restricted by hand, two index_select calls for
    the gather, three pair_matrix_device calls, the subtraction in torch, the members' matrices cleared with torch.  The baseline
    is not gated on the three verdicts (nothing a caller had could do that without a host read): the cheapest thing a caller
    could write, not an equivalent.  Also the members' scalars 18, 19 and 20 behind a binding matrix: 1 + 5 + 1 launches where
    scalar 19 is 3.
(c) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each (the children are scripts/decompose_timing.py's,
    which measure exactly that through the C ABI); each side's mean and its run-to-run spread (max - min).
`--evaluations` calls are enqueued on ONE stream of the caller's at one geometry per member with one synchronise per figure, the
kinds alternating over `--repeats` repeats.  Version 1, NoCutoff, Reference mode; every figure is a host clock around work that
ends in a synchronise.  This process only starts the children.  Prints tables and one JSON line with the library's build id.
What this script shares with scripts/decompose_group_timing.py is scripts/timing_support.py; here is what is the matrix's own.

  python scripts/pair_matrix_group_timing.py [--evaluations 2000] [--repeats 5] [--sizes 4,8] [--systems trpcage,1dwc]
                                             [--parent-library PATH [--parent-repeats 5]]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import timing_support  # noqa: E402


class Matrix:
    group, device, host = "pair_matrix_group", "pair_matrix_device", "pair_matrix"
    GROUP_HEADER = "| trpcage members | pair_matrix_group, us per call | the members' pair_matrix_device calls, us per round | per member: group / alone |"
    BINDING_HEADER = "| system | atoms (ligand), sets | binding pair_matrix_device, us | baseline, us |"

    def __init__(self, name):  # the residue partition of the system
        import openmm_agbnp_plugin_amd as P

        self.sets, labels = P.load_sets(os.path.join(ROOT, "tests", "golden", f"residues_{name}.txt"))
        self.S = len(labels)
        self.keys = dict(sets=self.S)

    def partition(self, obj, atoms=None):  # (a member's: the restriction, by hand, with the complex's numbering and S)
        obj.set_atom_sets(self.sets if atoms is None else self.sets[atoms], self.S)

    def shape(self, n):
        return (self.S, self.S)

    def members(self, sizes, f64):
        import torch

        return torch.zeros((len(sizes), self.S, self.S), **f64)

    def combine(self, d, m_mats, idx):  # the subtraction, the members' matrices cleared
        d.add_(m_mats[0] - m_mats[1] - m_mats[2])
        m_mats.zero_()

    def result_keys(self, d):
        return dict(matrix_sum=float(d.sum()))

    @staticmethod
    def group_note(got):
        return f"{got['sets']} sets; "

    @staticmethod
    def binding_cell(got):
        return f", {got['sets']}"

    @staticmethod
    def binding_note(got):
        return f"the matrix sums to {got['matrix_sum']:.6f}"


if __name__ == "__main__":
    timing_support.main("pair_matrix_group_timing.py", Matrix)
