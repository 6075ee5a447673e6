"""Kernel selection, the parts that need no GPU: which instantiations of the stepping kernels nk_engine.o holds (the rules the
pickers of nk_engine.hip prune by, stated once), that every kind nk_kind_normalise can return is one of them, and that the
statement macros the pickers replaced are gone."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(ROOT, 'nanokappa_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# k_sweep<GEOM, ROUGH, RBF, PID, SPLIT, LREC, FAST, BOX>
SWEEP = re.compile(r'^_Z7k_sweepILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d)ELb(\d)EEv5NkDevjii$')
_KERNELS = []


def _makefile_flags():
    """CXXFLAGS of nanokappa_amd/csrc/Makefile, expanded."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    base = re.search(r'^BASEFLAGS \?= (.*)$', mk, re.M).group(1)
    cxx = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1)
    return cxx.replace('$(BASEFLAGS)', base).split()


def _engine_kernels():
    """The kernels of nk_engine.hip's device code (one hipcc run, about a minute)."""
    if not _KERNELS:
        assert os.path.exists(HIPCC), 'hipcc is required here: the check is part of the build'
        tmp = tempfile.mkdtemp()
        try:
            out = os.path.join(tmp, 'nk_engine.s')
            subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + _makefile_flags() + ['--cuda-device-only', '-S', '-o', out,
                                                                                           os.path.join(CSRC, 'nk_engine.hip')], stderr=subprocess.DEVNULL)
            _KERNELS.extend(re.findall(r'^\s*\.amdhsa_kernel (\S+)', open(out).read(), re.M))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return _KERNELS


def _sweeps():
    return [tuple(int(x) for x in SWEEP.match(n).groups()) for n in _engine_kernels() if n.startswith('_Z7k_sweepI')]


def test_engine_object_holds_the_reachable_instantiations_and_no_others():
    k = _engine_kernels()
    assert len(k) == len(set(k)) == 132, len(k)
    assert len([n for n in k if n.startswith('_Z7k_sweepI')]) == 60
    assert len([n for n in k if n.startswith('_Z8k_eventsI')]) == 12
    assert len([n for n in k if n.startswith('_Z10k_residentI')]) == 8
    sweeps = _sweeps()
    assert len(set(sweeps)) == 60
    for geom, rough, rbf, pid, split, lrec, fast, box in sweeps:
        inst = 'k_sweep<%d, %d, %d, %d, %d, %d, %d, %d>' % (geom, rough, rbf, pid, split, lrec, fast, box)
        assert fast == 0, inst + ': the FAST sweeps live in nk_sweep_plain.o'
        assert pid or not rough, inst + ': rough facets imply ids'
        assert not (box and (geom == 2 or split)), inst + ': the box store needs tables in LDS and no split'


PROBE = r'''
#include <stdio.h>
#include "nk_kind.h"
int main() {
    for (int g = 0; g < 4; ++g) for (int f = 0; f < 4; ++f) for (int b = 0; b < 64; ++b) {
        const NkSweepKind k = nk_kind_normalise({g, (b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, f, (b & 32) != 0});
        printf("%d %d %d %d %d %d %d %d\n", k.geom, k.rough, k.rbf, k.pid, k.split, k.lrec, k.fast, k.box);
    }
    return 0;
}
'''


def test_every_normalised_kind_is_an_instantiation():
    """nk_kind_normalise over every raw kind (out-of-range geom and fast too): the kinds with FAST 0 are exactly the 60 sweeps of
    nk_engine.o, those with FAST 1 / 2 exactly the eight of nk_sweep_plain.hip."""
    tmp = tempfile.mkdtemp()
    try:
        src, exe = os.path.join(tmp, 'probe.hip'), os.path.join(tmp, 'probe')
        open(src, 'w').write(PROBE)
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-I' + CSRC, '-o', exe, src], stderr=subprocess.DEVNULL)
        kinds = set(tuple(int(x) for x in l.split()) for l in subprocess.check_output([exe]).decode().splitlines())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert set(k for k in kinds if k[6] == 0) == set(_sweeps())
    plain = open(os.path.join(CSRC, 'nk_sweep_plain.hip')).read()
    fast = set()
    for m in re.finditer(r'^template __global__ void k_sweep<([^>]*)>', plain, re.M):
        a = [x.strip() for x in m.group(1).split(',')] + ['false']                      # (BOX defaults to false)
        fast.add(tuple(int(x) if x.isdigit() else int(x == 'true') for x in a[:8]))
    assert len(fast) == 8 and set(k for k in kinds if k[6] != 0) == fast


def test_no_dispatch_macro_remains():
    for path in sorted(glob.glob(os.path.join(CSRC, '*'))):
        text = open(path, errors='replace').read() if os.path.isfile(path) and not path.endswith(('.o', '.s', '.so')) else ''
        hit = re.findall(r'NK_\w*_CASE\w*|NK_\w*_DISPATCH\w*', text)
        assert not hit, '%s: %s' % (os.path.basename(path), sorted(set(hit)))
