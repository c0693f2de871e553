#!/usr/bin/env python
"""One digest per function of the device code of each translation unit: two source trees whose lists agree give the GPU
the same code.  Each unit is compiled to gfx950 assembly with the build's own flags (cross-compiles without a GPU); the
text is cut at the compiler's "Begin function" / "End function" marks, so a kernel's digest covers its instructions, its
.amdhsa_kernel resource block, its register counts and its entry in the code-object metadata.  What depends on the file
rather than on the code is left out: .file / .ident lines, the __hip_cuid_* symbol, the order of the functions (local
labels are renumbered per function, the list is sorted).  The text is hashed, nothing in it is interpreted.
usage: python tools/asm_digest.py [--csrc DIR] [unit.hip ...]     (default: every unit of qcqp_amd/_build.py)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

_BEGIN = re.compile(r'-- Begin function (\S+)')
_END = re.compile(r'-- End function')
_LOCAL = re.compile(r'(\.L[A-Za-z_]+?|\bBB)(\d+)(?=_\d|\b)')     # (BB12_3 without .L: the loop comments of the assembly printer)
_PAD = re.compile(r'\s+;')
_SKIP = re.compile(r'^\s*\.(file|ident)\b|__hip_cuid_')


def _sha(lines):
    """Digest of a block of lines with its local labels (.LBB12_3, .Lfunc_end12, ...) renumbered by first appearance.  The
    function's number also stands in the printer's loop comments ("Header=BB12_3"), and its width sets the padding in front of
    them: a kernel that is the 99th function of one unit and the 100th of another has the same code."""
    seen = {}

    def renumber(m):
        key = (m.group(1), m.group(2))
        return '%s%d' % (m.group(1), seen.setdefault(key, len(seen)))

    return hashlib.sha256('\n'.join(_PAD.sub(' ;', _LOCAL.sub(renumber, l)) for l in lines).encode()).hexdigest()[:16]


def assembly(path, include):
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-I' + include]     # _build.py's
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'unit.s')
        subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + flags + ['--cuda-device-only', '-S', path, '-o', out],
                       check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def digests(text):
    """{function name: digest}; '(module)' stands for everything outside the functions (variables, target, version)."""
    lines = [l.rstrip() for l in text.splitlines() if not _SKIP.search(l)]
    funcs, rest, meta, cur, name, in_meta, in_list = {}, [], {}, None, None, False, True
    for l in lines:
        if in_meta:
            if l and not l.startswith(' '):     # the kernel list is over: target, version
                cur, in_list = None, False
            elif l.startswith('  - ') and in_list:
                cur = []
                meta[len(meta)] = cur
            (cur if cur is not None else rest).append(l)
            continue
        if l.startswith('amdhsa.kernels:'):
            in_meta, cur = True, None
            rest.append(l)
            continue
        m = _BEGIN.search(l)
        if m and cur is None:
            name, cur = m.group(1), []
        (cur if cur is not None else rest).append(l)
        if cur is not None and _END.search(l):
            funcs[name], cur = cur, None
    for entry in meta.values():     # the metadata entry of a kernel joins the kernel's text
        kname = [l.split(':', 1)[1].strip() for l in entry if l.strip().startswith('.name:')][0]
        funcs[kname] = funcs[kname] + entry
    out = {n: _sha(b) for n, b in funcs.items()}
    out['(module)'] = _sha(rest)
    return out


def main():
    args = sys.argv[1:]
    csrc = os.path.join(REPO, 'qcqp_amd', 'csrc')
    if args[:1] == ['--csrc']:
        csrc, args = os.path.abspath(args[1]), args[2:]
    if not args:
        from qcqp_amd._build import TRANSLATION_UNITS
        args = TRANSLATION_UNITS
    include = os.path.join(os.path.dirname(os.path.dirname(csrc)), 'include')
    with ThreadPoolExecutor(max_workers=8) as ex:
        texts = list(ex.map(lambda u: assembly(os.path.join(csrc, u), include), args))
    for unit, text in zip(args, texts):
        for n, d in sorted(digests(text).items()):
            print('%s  %s  %s' % (d, unit, n))


if __name__ == '__main__':
    main()
