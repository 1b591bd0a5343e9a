"""Child process of test_attention_layouts_gpu.py::test_attention_switches_are_bit_identical: runs the training attention on long-block layouts of
tests/_attn_cases.py under the TFX_ATTN_* switches of its environment (the library reads them once per process) and prints one line of sha256s
(out, lse, d q~ | d k~, d v | d gate) per case and plan mode."""
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from _attn_cases import CASES, run_kernels  # noqa: E402


def h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def main():
    for name in ('n129', 'n1000', 'n2048', 'dh32'):
        for mode in (None, 0, 1):
            _, _, got = run_kernels(CASES[name], mode)
            r = got['raw']
            print(f'CASE {name} mode={mode} ' + ' '.join(f'{k}={h(v)}' for k, v in r.items()), flush=True)


if __name__ == '__main__':
    main()
