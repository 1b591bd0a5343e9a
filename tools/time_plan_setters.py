"""Host time of the per-structure setters of a training Plan - set_segments + set_rope_tables + set_rows - on a CPU-built plan of depth 24 (dim 64,
tests/_plan_digest.cpu_plan), after one build and after eight distinct frozen sets went through select_frozen.  No GPU.

    python tools/time_plan_setters.py [TREE]        # TREE: the checkout to measure (default: this one); run it on two trees in turn to compare them

Prints the CPU time per call of the three setters together, in microseconds, for seven rounds of 3000 calls, sorted."""
import os
import sys
import time

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TREE, os.path.join(TREE, 'tests')]

import torch  # noqa: E402
import _plan_digest as P  # noqa: E402

assert os.path.samefile(P.ROOT, TREE), (P.ROOT, TREE)
torch.set_num_threads(1)
m, ps, plan = P.cpu_plan(depth=24)
seg = (torch.tensor([0, 64], dtype=torch.int32), torch.tensor([64, 64], dtype=torch.int32))
rope = (torch.ones(64, 32), torch.zeros(64, 32))


def rounds(n=3000, reps=7):
    out = []
    for _ in range(reps):
        t0 = time.process_time()
        for _ in range(n):
            plan.set_segments(*seg); plan.set_rope_tables(*rope); plan.set_rows({0: 8, 1: 4})
        out.append((time.process_time() - t0) / n * 1e6)
    return ' '.join(f'{x:.1f}' for x in sorted(out))


print('after one build          us per call:', rounds())
for k in range(8):
    plan.select_frozen(frozenset(n for n in ps.params if f'.layers.{k}.' in n and '.2.fn.' in n))
print('after eight frozen sets  us per call:', rounds())
