"""Kernel-by-kernel comparison of the gfx950 device assembly of two source trees (a refactor's "same ISA" check).

usage: python tools/isa_compare.py BASE_TREE [HEAD_TREE]      (HEAD_TREE defaults to this checkout)
       python tools/isa_compare.py --asm BASE_DIR HEAD_DIR     (directories of <source>.hip.s files compiled already)

Compiles every csrc/*.hip of both trees with build.py's FLAGS plus --cuda-device-only -S, then, per source file and kernel:
  same       instructions and resources identical
  kernarg    identical except the immediate offsets of scalar loads and .amdhsa_kernarg_size (an argument struct shrank)
  renamed    no kernel of that name in HEAD, but one with an identical body (a template parameter went)
  DIFFERENT  anything else, with the first differing lines
  removed    no counterpart in HEAD
Resources (VGPR / SGPR / AGPR counts, LDS, scratch) must match for every kernel that is not removed.  Exit status 1 on any
DIFFERENT kernel or resource mismatch."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-Wno-unused-result']
RES = ('num_vgpr', 'num_agpr', 'numbered_sgpr', 'private_seg_size', 'uses_vcc', 'uses_flat_scratch', 'has_dyn_sized_stack',
       '.amdhsa_next_free_vgpr', '.amdhsa_next_free_sgpr', '.amdhsa_accum_offset', '.amdhsa_group_segment_fixed_size',
       '.amdhsa_private_segment_fixed_size')


def assemble(tree, out):
    csrc = os.path.join(tree, '3d-object-detection.pytorch_amd', 'csrc')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith('.hip'))

    def cc(s):
        subprocess.run([hipcc, *FLAGS, '--cuda-device-only', '-S', os.path.join(csrc, s), '-o', os.path.join(out, s + '.s')],
                       check=True, capture_output=True)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(cc, srcs))
    return srcs


def kernels(path):
    """{mangled name: [normalised body lines, {resource: value}]}: instructions and kernel descriptor, without labels' numbers,
    comments, the kernel's own name and .amdhsa_kernarg_size (kept as a resource)"""
    text = open(path).read().split('\n')
    out = {}
    for i, line in enumerate(text):
        m = re.match(r'^(\S+):\s*(;.*)?$', line)
        if m and i > 0 and text[i - 1].strip().startswith('.type') and '@function' in text[i - 1]:
            name, body, res = m.group(1), [], {}
            j = i + 1
            while not text[j].startswith('.Lfunc_end'):
                ln = text[j].split(';')[0].strip()
                f = ln.split()
                if f and f[0] in RES + ('.amdhsa_kernarg_size',):
                    res[f[0]] = f[1]
                if ln and not ln.startswith(('.amdhsa_kernel', '.amdhsa_kernarg_size')):
                    body.append(re.sub(r'\.LBB\d+_', '.LBB_', ln).replace(name, '<self>'))
                j += 1
            out[name] = [body, res]
        m = re.match(r'^\s*\.set (\S+)\.(\w+), (\S+)', line)
        if m and m.group(1) in out:
            out[m.group(1)][1][m.group(2)] = m.group(3)
    return out


def masked(body):
    """immediate offsets of scalar loads and of scalar address adds (kernel-argument addresses) -> <off>"""
    return [re.sub(r'^((?:s_load_\S+|s_add_u32)\s+[^,]+,\s*[^,]+,\s*)0x[0-9a-f]+$', r'\1<off>', ln) for ln in body]


def compare(ob, oh):
    sb = sorted(f[:-2] for f in os.listdir(ob) if f.endswith('.hip.s'))
    sh = set(f[:-2] for f in os.listdir(oh) if f.endswith('.hip.s'))
    bad, counts = 0, {}
    for s in sb:
        kb = kernels(os.path.join(ob, s + '.s'))
        kh = kernels(os.path.join(oh, s + '.s')) if s in sh else {}
        unmatched = dict(kh)
        for name, (body, res) in kb.items():
            if name in kh:
                hbody, hres = kh[name]
                unmatched.pop(name, None)
                verdict = 'same' if body == hbody else ('kernarg' if masked(body) == masked(hbody) else 'DIFFERENT')
            else:
                # (the candidate whose name shares the longest prefix first: template instances can compile to equal code)
                cands = sorted(unmatched, key=lambda n: -len(os.path.commonprefix([n, name])))
                hit = next((n for n in cands if masked(unmatched[n][0]) == masked(body)), None)
                if hit is None:
                    counts['removed'] = counts.get('removed', 0) + 1
                    print(f'removed    {s}: {name}')
                    continue
                hbody, hres = unmatched.pop(hit)
                verdict = 'renamed'
                print(f'renamed    {s}: {name} -> {hit}' + ('' if body == hbody else ' (kernarg offsets differ)'))
            counts[verdict] = counts.get(verdict, 0) + 1
            rdiff = {k: (res.get(k), hres.get(k)) for k in RES if res.get(k) != hres.get(k)}
            if verdict == 'DIFFERENT' or rdiff:
                bad += 1
                print(f'{verdict:10s} {s}: {name}  resources {rdiff}')
                if verdict == 'DIFFERENT':
                    diff = [(a, b) for a, b in zip(masked(body), masked(hbody)) if a != b][:5]
                    print(f'    {len(body)} vs {len(hbody)} lines; first differences: {diff}')
            elif verdict == 'kernarg':
                print(f'kernarg    {s}: {name}  kernarg size {res.get(".amdhsa_kernarg_size")} -> '
                      f'{hres.get(".amdhsa_kernarg_size")}')
        for name in unmatched:
            print(f'new        {s}: {name}')
            bad += 1
    print('summary:', ', '.join(f'{k} {v}' for k, v in sorted(counts.items())), f'-- {bad} problem(s)')
    return bad


def main():
    if sys.argv[1] == '--asm':
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    base = os.path.abspath(sys.argv[1])
    head = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(HERE)
    with tempfile.TemporaryDirectory() as tmp:
        ob, oh = os.path.join(tmp, 'base'), os.path.join(tmp, 'head')
        os.makedirs(ob)
        os.makedirs(oh)
        assemble(base, ob)
        assemble(head, oh)
        sys.exit(1 if compare(ob, oh) else 0)


if __name__ == '__main__':
    main()
