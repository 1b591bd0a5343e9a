#!/bin/bash
# register budget of every kernel (VGPRs, spills, LDS): run after ANY kernel edit - a spilling hot loop costs more than any schedule gains
# usage: bash tools/check_spills.sh            kernels that spill or take more than 128 VGPRs
#        bash tools/check_spills.sh --all      every kernel, with SGPRs, scratch bytes, the number of instructions and a digest of its assembly text: a listing to
#                                              join by kernel name with the same listing of another revision (equal digests = the same instruction stream).
#                                              The digest is of the text between the kernel's label and the end of the function, normalised so that it is
#                                              comparable across revisions: the compiler's comments (from `;` to the end of the line) and the lines they leave
#                                              empty are dropped, the per-file function index of local labels (.LBB<n>_) becomes a fixed token, and so does
#                                              the kernel's own mangled name - all three change when another kernel of the file comes or goes, or when a
#                                              template parameter list changes.  profiles/attn_fwd_asm_removed.txt is such a join; digests from before this
#                                              normalisation, such as those in profiles/tokenwise_row_helpers.txt, were computed on the raw text
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
for f in gemm attention tokenwise lora muon decode; do
  FF=""; [ $f = attention ] && FF="-fno-slp-vectorize"      # build.py FILE_FLAGS
  (cd $R/transfusion_pytorch_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -fPIC $FF -I../../include -c $f.hip -o $T/$f.o -save-temps=obj 2>/dev/null)
done
python3 - $T "$1" <<'PY'
import re, sys, glob, hashlib
bad = 0
every = sys.argv[2] == '--all'
for path in sorted(glob.glob(sys.argv[1] + '/*gfx950.s')):
    txt = open(path).read()
    count, body = {}, {}                           # per kernel: the lines between its label and the end of the function; those that start with a mnemonic are counted
    if every:
        cur = None
        for ln in txt.split('\n'):
            m = re.match(r'^(_Z\w+):', ln)
            if m and cur is None: cur = m.group(1); count[cur] = 0; body[cur] = hashlib.md5()
            elif cur and ln.startswith('.Lfunc_end'): cur = None
            elif cur:
                norm = re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip()).replace(cur, 'KERNEL')
                if norm: body[cur].update(norm.encode() + b'\n')
                if re.match(r'^\s+[a-z]', ln): count[cur] += 1
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_count:\s*(\d+).*?\.vgpr_count:\s*(\d+)\s*\n\s*\.vgpr_spill_count:\s*(\d+)', txt, re.S):
        lds, name, priv, sg, vg, sp = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))
        short = re.sub(r'^_ZN3tfx\d+', '', name)
        flag = '  <-- SPILLS' if sp else ''
        if sp: bad += 1
        dig = body[name].hexdigest()[:8] if name in body else '-'
        if every: print(f'{short[:88]:90s} vgpr {vg:3d} sgpr {sg:3d} spill {sp:3d} scratch {priv:4d} lds {lds:6d} insn {count.get(name, 0):5d} asm {dig}{flag}')
        elif sp or vg > 128: print(f'{short[:60]:62s} vgpr {vg:3d} spill {sp:3d} lds {lds}{flag}')
print('kernels with spills:', bad)
PY
rm -rf $T
