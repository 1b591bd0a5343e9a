"""The text draw's launch alone: tfx_sample_tokens_range against tfx_sample_tokens_filtered (include/tfx.h) with the filters off, top-k, top-p and both.
   python tools/bench_sampler_filters.py [--batch 64 --rounds 5 --launches 200]
Per setting and vocabulary: microseconds per launch = device-event time over `--launches` back-to-back launches on one stream (kernel time plus the gap
to the next launch; not a profiler's kernel time), in `--rounds` rounds that alternate the settings - minimum, median and maximum over the rounds.
The ids of "off" are compared with the old entry's before anything is timed."""
import argparse, ctypes, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transfusion_pytorch_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64); ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--launches', type=int, default=200)
ap.add_argument('--vocab', type=int, nargs='+', default=[264, 32000], help='row widths: 264 = the examples\' 256 text tokens + meta tokens; 32 000 = tools/bench_text_head.py')
ap.add_argument('--temperature', type=float, default=1.); ap.add_argument('--min-p', type=float, default=0.1)
a = ap.parse_args()
L, B = capi.lib(), a.batch
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
# row passes (header): maximum 1 + top-k 8 + (M 1 + top-p 8) + mass 1 + scan 1
SETTINGS = [('range (old entry)', None, None, 3), ('filtered, off', 0, 1., 3), ('filtered, top-k 40', 40, 1., 11), ('filtered, top-p 0.9', 0, 0.9, 12),
            ('filtered, top-k 40 + top-p 0.9', 40, 0.9, 20)]
for V in a.vocab:
    g = torch.Generator(device='cuda').manual_seed(0)
    ld = (V + 7) // 8 * 8
    lg = torch.randn(B, ld, device='cuda', generator=g) * 3.
    u = torch.rand(B, device='cuda', generator=g)
    out = torch.empty(B, dtype=torch.int32, device='cuda')

    def launch(k, p):
        if k is None:
            rc = L.tfx_sample_tokens_range(lg.data_ptr(), ld, B, V, V, a.temperature, a.min_p, u.data_ptr(), None, out.data_ptr(), stream)
        else:
            rc = L.tfx_sample_tokens_filtered(lg.data_ptr(), ld, B, V, V, a.temperature, a.min_p, k, p, u.data_ptr(), None, out.data_ptr(), stream)
        capi.check(rc, 'sampler launch')

    ids = {}
    for name, k, p, _ in SETTINGS:                                   # warm-up of every setting, and what each draws
        launch(k, p); torch.cuda.synchronize(); ids[name] = out.clone()
    assert torch.equal(ids[SETTINGS[0][0]], ids[SETTINGS[1][0]]), 'filters off must draw what the old entry draws'
    times = {name: [] for name, *_ in SETTINGS}
    for _ in range(a.rounds):
        for name, k, p, _ in SETTINGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch(k, p)
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    print(f'V = {V} (ld {ld}), batch {B}, temperature {a.temperature}, min_p {a.min_p}; {a.rounds} alternated rounds x {a.launches} launches, us per launch')
    for name, k, p, passes in SETTINGS:
        t = times[name]
        same = int((ids[name] == ids[SETTINGS[0][0]]).sum())
        print(f'  {name:34s} {passes:2d} row passes   min {min(t):8.2f}  median {statistics.median(t):8.2f}  max {max(t):8.2f}   ({same} of {B} ids as the old entry)')
