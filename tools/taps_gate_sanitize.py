#!/usr/bin/env python3
"""The tap-table gate under the host sanitizers: a stand-alone program, on the CPU only.

Builds ``csrc/vnd_amd.hip`` into a temporary directory with AddressSanitizer and UndefinedBehaviorSanitizer on the HOST
side (``-Xarch_host -fsanitize=address,undefined``, undefined behaviour fatal), writes the refusal corpus of
``tests/taps_gate.py`` (every malformed table and image of the CPU tier, the refused mutants included) to a data file,
compiles ``tools/micro/taps_gate_main.cpp`` with the same sanitizers, links it against that library and runs it.  The
program has its own ``main``: nothing is preloaded, nothing is loaded into Python.  Every case is refused before the gate
would touch a device, so this needs no GPU - run it on a machine without one; it is not a test of the suite.

    python tools/taps_gate_sanitize.py [--source DIR] [--keep DIR] [--skip TEXT ...]

``--source DIR``: a checkout whose ``vndecorrelate_amd/csrc`` and ``include`` are built instead of this one's (the
corpus and the program stay this tree's) - how the report of an older commit is taken.  Exit status 0: every case
refused as the mirror predicts and no sanitizer report.  The first report ends the program: ``--skip TEXT`` leaves out
the cases whose name contains TEXT, to see what an older commit reports after its first finding.  The library build
takes about two minutes; ``--keep DIR`` reuses the one already in DIR.
"""
import argparse
import os
import pathlib
import shutil
import struct
import subprocess
import sys
import tempfile

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'tests')]
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']


def corpus_bytes(skip=()) -> bytes:
    import taps_gate as G

    def padded(raw: bytes) -> bytes:
        return raw + b'\0' * (-len(raw) % 4)

    cases = [c for c in G.refusal_corpus() if not any(text in c.name for text in skip)]
    out = [struct.pack('<2i', 0x474E4456, len(cases))]
    for c in cases:
        if c.entry == 'create':
            t = c.table
            out.append(struct.pack('<6i', 0, c.verdict.status, c.null_out, c.null_ctx, t.C, t.apply_gain))
            for a in (t.tap_offsets, t.tap_index, t.tap_weight, t.seg_offsets, t.seg_end, t.seg_gain, t.chan_flags):
                raw = b'' if a is None else a.tobytes()
                out.append(struct.pack('<2i', a is not None, len(raw)) + padded(raw))
        else:
            raw = c.image or b''
            nbytes = len(raw) if c.nbytes is None else c.nbytes
            out.append(struct.pack('<8i', 1, c.verdict.status, c.null_out, c.null_ctx, c.misaligned, c.image is not None,
                                   nbytes, len(raw)) + padded(raw))
    return b''.join(out)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--source', type=pathlib.Path, default=REPO, help='checkout whose library sources are built')
    ap.add_argument('--keep', type=pathlib.Path, help='build here and keep the products (default: a temporary directory)')
    ap.add_argument('--skip', action='append', default=[], metavar='TEXT', help='leave out the cases whose name contains TEXT')
    args = ap.parse_args()
    import __graft_entry__ as entry
    hipcc = entry._hipcc()
    rocm = pathlib.Path(shutil.which(hipcc) or hipcc).resolve().parent.parent          # hipcc lives in <rocm>/bin
    csrc, include = args.source / 'vndecorrelate_amd' / 'csrc', args.source / 'include'
    with tempfile.TemporaryDirectory(prefix='taps_gate_san_') as tmp:
        work = args.keep or pathlib.Path(tmp)
        work.mkdir(parents=True, exist_ok=True)
        lib, prog, data = work / 'libvnd_amd_san.so', work / 'taps_gate_main', work / 'corpus.bin'
        data.write_bytes(corpus_bytes(args.skip))
        if not (args.keep and lib.exists()):
            xhost = [flag for s in SANITIZE for flag in ('-Xarch_host', s)]
            cmd = [hipcc, *entry.HIPCC_FLAGS, '-g', *xhost, str(csrc / 'vnd_amd.hip'), '-o', str(lib), '-lhiprtc', '-ldl']
            print('building', lib.name, '...', flush=True)
            subprocess.run(cmd, check=True, cwd=str(args.source))
        cxx = os.environ.get('CXX') or str(rocm / 'llvm' / 'bin' / 'clang++')
        subprocess.run([cxx, '-std=c++17', '-g', '-O1', *SANITIZE, '-I', str(include), str(REPO / 'tools' / 'micro' / 'taps_gate_main.cpp'),
                        '-o', str(prog), f'-L{work}', '-lvnd_amd_san', f'-Wl,-rpath,{work}', f'-Wl,-rpath,{rocm / "lib"}'], check=True)
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
        done = subprocess.run([str(prog), str(data)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(done.stdout, end='')
        print(f'taps_gate_sanitize: exit status {done.returncode}' + ('' if done.returncode else ' - clean'))
        return done.returncode


if __name__ == '__main__':
    sys.exit(main())
