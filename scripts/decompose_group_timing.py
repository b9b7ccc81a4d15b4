#!/usr/bin/env python3
"""What decomposition groups and the per-atom decomposition of a binding energy cost (include/agbnp_hip.h:
agbnp_hip_decompose_group, agbnp_hip_binding_decompose_device), beside what a caller could write before they
existed, and that adding them has left the full evaluation alone.

(a) One child process per group size: microseconds per decompose_group() call over R trpcage contexts, and per round of the same
    members' R decompose_device() calls back to back, in the same process.
(b) One child process per system: microseconds per BindingEnergy.decompose_device() call, and per call of the BASELINE in the
    same process -- three contexts (complex, receptor, ligand), two index_select calls for the gather, three decompose_device
    calls, the scatter and the subtraction in torch, the members' planes cleared with torch.  The baseline is not gated on the
    three verdicts (nothing a caller had could do that without a host read): the cheapest thing a caller could write, not an
    equivalent.  Also the members' scalars 18, 19 and 20 behind a binding decomposition: 1 + 5 + 1 launches where scalar 19 is 3.
(c) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each (the children are scripts/decompose_timing.py's,
    which measure exactly that through the C ABI); each side's mean and its run-to-run spread (max - min).
`--evaluations` calls are enqueued on ONE stream of the caller's at one geometry per member with one synchronise per figure, the
kinds alternating over `--repeats` repeats.  Version 1, NoCutoff, Reference mode; every figure is a host clock around work that
ends in a synchronise.  This process only starts the children.  Prints tables and one JSON line with the library's build id.
What this script shares with scripts/pair_matrix_group_timing.py is scripts/timing_support.py; here is what is the planes' own.

  python scripts/decompose_group_timing.py [--evaluations 2000] [--repeats 5] [--sizes 4,8] [--systems trpcage,1dwc]
                                           [--parent-library PATH [--parent-repeats 5]]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import timing_support  # noqa: E402


class Planes:
    group, device, host = "decompose_group", "decompose_device", "decompose"
    GROUP_HEADER = "| trpcage members | decompose_group, us per call | the members' decompose_device calls, us per round | per member: group / alone |"
    BINDING_HEADER = "| system | atoms (ligand) | binding decompose_device, us | baseline, us |"
    keys = {}

    def __init__(self, name):
        pass

    def partition(self, obj, atoms=None):
        pass

    def shape(self, n):
        return (4, n)

    def members(self, sizes, f64):
        import torch

        return [torch.zeros(self.shape(n), **f64) for n in sizes]

    def combine(self, terms, m_terms, idx):  # the scatter and the subtraction, the members' planes cleared
        terms.add_(m_terms[0])
        for m in (1, 2):
            terms.index_add_(1, idx[m], m_terms[m], alpha=-1.0)
        for t in m_terms:
            t.zero_()

    def result_keys(self, terms):
        return dict(plane_totals=[float(x) for x in terms.sum(axis=1)])

    group_note = binding_cell = staticmethod(lambda got: "")

    @staticmethod
    def binding_note(got):
        return f"plane totals {got['plane_totals']}"


if __name__ == "__main__":
    timing_support.main("decompose_group_timing.py", Planes)
