"""Replica groups, the parts that need no GPU: --replicas and the seeds it stands for, the folder layout, the statistics over the
replicas on synthetic convergence rows, the C interface, and the shape of the group kernels in the gfx950 assembly."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(ROOT, 'nanokappa_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'nanokappa_hip.h')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
REQ = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic']


# ---------------------------------------------------------------------------------------------- 1. the command line
def test_replicas_option_and_seeds():
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.ensemble import replica_seeds
    p = initialise_parser()
    a = p.parse_args(REQ)
    assert a.replicas == [1] and replica_seeds(a.seed, a.replicas) == [0]           # the default: one run, its own seed
    a = p.parse_args(REQ + ['--replicas', '8', '--seed', '2025'])
    assert a.replicas == [8]
    assert replica_seeds(a.seed, a.replicas) == list(range(2025, 2033))
    assert replica_seeds(7, 3) == [7, 8, 9]
    with pytest.raises(ValueError, match='--replicas'):
        replica_seeds([0], [0])
    with pytest.raises(SystemExit):
        p.parse_args(REQ + ['--replicas', 'many'])


def test_replica_arguments_and_folders(tmp_path):
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.ensemble import replica_args, replica_folder
    a = initialise_parser().parse_args(REQ + ['--seed', '5', '--replicas', '3'])
    a.results_folder = str(tmp_path / 'run_0')
    os.makedirs(a.results_folder)
    for k, s in enumerate((5, 6, 7)):
        r = replica_args(a, s, k)
        assert r.seed == [s] and r.results_folder == os.path.join(a.results_folder, 'replica_%d' % k)
        assert os.path.isdir(r.results_folder)
        assert r.particles == a.particles and r is not a
    assert a.seed == [5] and a.results_folder == str(tmp_path / 'run_0')               # the caller's arguments are untouched
    assert sorted(os.listdir(a.results_folder)) == ['replica_0', 'replica_1', 'replica_2']
    assert replica_folder('', 2) == ''                                                 # no folder: no files, as for a Population


# ---------------------------------------------------------------------------------------------- 2. the statistics
def fake_population(rng, n_rows, S, n_mean, kappa0):
    rows = []
    for _ in range(n_rows):
        rows.append(dict(T=300.0 + rng.normal(size=S), phi=rng.normal(size=(S, 3)), en_res=rng.normal(size=2),
                         sv_k=kappa0 + rng.normal(size=S), kappa=kappa0 + rng.normal()))
    return types.SimpleNamespace(n_mean=n_mean, conv_rows=rows, subvol_type='slice')


def test_summary_statistics_on_synthetic_rows(tmp_path):
    from nanokappa_amd.ensemble import replica_statistics, summarise, across_replicas, write_summary, read_summary
    rng = np.random.default_rng(3)
    S, n_mean, R = 5, 12, 4
    pops = [fake_population(rng, 40, S, n_mean, 100.0 + k) for k in range(R)]
    per = [replica_statistics(p) for p in pops]
    # per replica: mean and std over the LAST n_mean rows
    for p, st in zip(pops, per):
        kk = np.array([r['kappa'] for r in p.conv_rows[-n_mean:]])
        assert st['kappa'][0][0] == np.mean(kk) and st['kappa'][1][0] == np.std(kk)
        T = np.array([r['T'] for r in p.conv_rows[-n_mean:]])
        assert np.array_equal(st['T_sv'][0], T.mean(axis=0)) and np.array_equal(st['T_sv'][1], T.std(axis=0))
        assert st['phi'][0].shape == (3 * S,)
    s = summarise(per)
    kap = np.array([st['kappa'][0][0] for st in per])
    assert s['kappa']['mean'][0] == np.mean(kap)
    assert s['kappa']['std'][0] == np.std(kap, ddof=1)
    assert s['kappa']['sem'][0] == np.std(kap, ddof=1) / np.sqrt(R)
    Tm = np.array([st['T_sv'][0] for st in per])
    assert np.array_equal(s['T_sv']['mean'], Tm.mean(axis=0)) and np.array_equal(s['T_sv']['std'], Tm.std(axis=0, ddof=1))
    assert np.array_equal(s['T_sv']['sem'], Tm.std(axis=0, ddof=1) / np.sqrt(R))
    m, sd, se = across_replicas(np.array([[1.0], [2.0], [4.0]]))
    assert m[0] == 7.0 / 3.0 and sd[0] == np.std([1.0, 2.0, 4.0], ddof=1) and se[0] == sd[0] / np.sqrt(3.0)
    m, sd, se = across_replicas(np.array([[1.0, 2.0]]))                                # one replica: a mean, no error bar
    assert np.array_equal(m, [1.0, 2.0]) and np.all(np.isnan(sd)) and np.all(np.isnan(se))
    # ensemble.txt reads back to the same numbers
    path = str(tmp_path / 'ensemble.txt')
    write_summary(path, s, [10, 11, 12, 13], False, 'member 0 is outside the grouped path: it has rough facets')
    back = read_summary(path)
    assert back['kappa'].shape == (1, 3 + 2 * R) and back['T_sv'].shape == (S, 3 + 2 * R) and back['phi'].shape == (3 * S, 3 + 2 * R)
    assert back['kappa'][0, 0] == s['kappa']['mean'][0] and back['kappa'][0, 1] == s['kappa']['std'][0]
    assert np.array_equal(back['T_sv'][:, 2], s['T_sv']['sem'])
    assert np.array_equal(back['kappa'][0, 3::2], kap)
    head = open(path).read().splitlines()
    assert head[0] == '# replicas 4  seeds 10 11 12 13' and head[1].startswith('# grouped no: member 0') and 'rough' in head[1]


def test_population_run_is_plan_then_consume():
    """Population.run is the loop over its two halves that Ensemble.run drives for several populations."""
    import inspect
    from nanokappa_amd.population import Population
    from nanokappa_amd.ensemble import Ensemble
    src = inspect.getsource(Population.run)
    assert '_plan_chunk' in src and '_consume_chunk' in src and 'self.engine.step(chunk)' in src
    src = inspect.getsource(Ensemble.run)
    assert '_plan_chunk' in src and '_consume_chunk' in src and 'self.group.step(chunk)' in src


# ---------------------------------------------------------------------------------------------- 3. the C interface
GROUP_SYMBOLS = ('nk_group_create', 'nk_group_destroy', 'nk_group_step', 'nk_group_info', 'nk_group_last_error')


def test_header_stays_plain_c():
    subprocess.check_call(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', HEADER])
    hdr = open(HEADER).read()
    assert 'typedef struct nk_group nk_group;' in hdr
    assert 'int nk_group_create(nk_group **out, nk_ctx *const *members, int32_t R);' in hdr
    assert 'int nk_group_step(nk_group *g, int32_t nsteps, nk_tally *outs' in hdr
    assert '#define NK_GROUP_MAX_MEMBERS 32' in hdr


def test_group_symbols_are_declared_and_exported():
    from nanokappa_amd import engine
    hdr = open(HEADER).read()
    for n in GROUP_SYMBOLS:
        assert n in engine.EXPORTS and n + '(' in hdr
    assert engine.GROUP_MAX_MEMBERS == 32 and engine.ERR_ARG == -2
    # nk_group_report as the header lays it out: six int32, four int64, three doubles; nk_timing keeps its layout
    assert C.sizeof(engine.nk_group_report) == 6 * 4 + 4 * 8 + 3 * 8
    assert C.sizeof(engine.nk_timing) == 15 * 8
    fields = re.search(r'typedef struct \{([^}]*)\} nk_group_report;', hdr, re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = re.findall(r'(\w+);', fields)
    assert names == [k for k, _ in engine.nk_group_report._fields_]
    assert hasattr(engine, 'EngineGroup')


def test_makefile_links_the_group_objects_everywhere():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'GROUP_OBJS := nk_group.o nk_group_plain.o' in mk
    for target in ('$(OUT)', 'stamps', 'stats', 'variant'):
        rule = re.search(r'^%s:.*\n(?:\t.*\n)+' % re.escape(target), mk, re.M).group(0)
        assert '$(GROUP_OBJS)' in rule.split('\n')[0], target
        assert '$(GROUP_OBJS) -ldl' in rule, target
    # the FAST sweeps with the flags of nk_sweep_plain.o, the rest with the library's
    assert re.search(r'^nk_group_plain\.o:.*\n\t.*\$\(BASEFLAGS\) -DNK_GROUP_PLAIN ', mk, re.M)
    assert re.search(r'^nk_group\.o:.*\n\t.*\$\(CXXFLAGS\) ', mk, re.M)


# ---------------------------------------------------------------------------------------------- 4. the shape of the kernels
BASEFLAGS = ['-O3', '-std=c++17', '-munsafe-fp-atomics']
_ASM = {}


def _assembly(which):
    """'group': nk_group.hip with the library's flags (machine LICM off); 'group_plain': the same file, -DNK_GROUP_PLAIN, with the
    flags of nk_sweep_plain.hip; 'sweep_plain': nk_sweep_plain.hip, the solo kernels the FAST group sweeps mirror."""
    if which not in _ASM:
        assert os.path.exists(HIPCC), 'hipcc is required here: the check is part of the build'
        src, flags = {'group': ('nk_group.hip', ['-mllvm', '-disable-machine-licm']),
                      'group_plain': ('nk_group.hip', ['-DNK_GROUP_PLAIN']),
                      'sweep_plain': ('nk_sweep_plain.hip', [])}[which]
        tmp = tempfile.mkdtemp()
        try:
            out = os.path.join(tmp, which + '.s')
            subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + BASEFLAGS + flags + ['--cuda-device-only', '-S', '-o', out,
                                                                                         os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)
            _ASM[which] = open(out).read()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return _ASM[which]


def _kernels(text):
    """name -> (instructions, metadata block) of every kernel in an assembly file."""
    out = {}
    lines = text.split('\n')
    for name in re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, re.M):
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
        b = next(i for i in range(a, len(lines)) if '.end_amdhsa_kernel' in lines[i])
        code = [l.split(';')[0].strip() for l in lines[a:b]]
        out[name] = ([c.split()[0] for c in code if c and not c.startswith('.') and not c.endswith(':')], '\n'.join(lines[a:b]))
    return out


def _vgprs(meta):
    return int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', meta).group(1))


def _check_group_kernel(name, ops, meta):
    assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', meta), name + ': scratch'
    assert not [o for o in ops if o.startswith('scratch_')], name + ': scratch operations'
    # the members' NkDevs, the prefix table and the records are read with scalar loads (constant address space)
    assert [o for o in ops if o.startswith('s_load_dword')], name


def test_group_kernels_hold_nothing_else_and_use_no_scratch():
    k = _kernels(_assembly('group'))
    sweeps = [n for n in k if 'k_sweep_group' in n]
    tails = [n for n in k if 'k_tail_group' in n]
    assert len(sweeps) == 8 and len(tails) == 2 and len(k) == 10, sorted(k)        # PID x LREC x BOX sweeps, BOX tails: nothing else
    for n in sweeps + tails:
        _check_group_kernel(n, *k[n])
    # the FAST = 0 sweeps mirror k_sweep<1, false, false, PID, false, LREC, 0, BOX> of nk_engine.o (launch bounds: three workgroups of
    # four waves per CU): within that occupation bound, 512 / 3 -> 168 VGPRs
    for n in sweeps:
        assert _vgprs(k[n][1]) <= 168, '%s: %d VGPRs' % (n, _vgprs(k[n][1]))
    kp = _kernels(_assembly('group_plain'))
    assert len(kp) == 8 and all('k_sweep_group' in n for n in kp), sorted(kp)      # LREC x FAST 1 / 2 x BOX
    for n in kp:
        _check_group_kernel(n, *kp[n])


def test_fast_group_sweep_needs_no_more_registers_than_the_sweep_it_mirrors():
    """k_sweep_group<false, LREC, FAST, BOX> against k_sweep<1, false, false, false, false, LREC, FAST, BOX>, both compiled here with
    the same flags: no more VGPRs, so the same workgroups per CU."""
    group = _kernels(_assembly('group_plain'))
    solo = _kernels(_assembly('sweep_plain'))
    assert len([n for n in solo if n.startswith('_Z7k_sweepI')]) == 8
    pairs = 0
    for lrec in (0, 1):
        for fast in (1, 2):
            for box in (0, 1):
                g = [n for n in group if 'k_sweep_groupILb0ELb%dELi%dELb%dE' % (lrec, fast, box) in n]
                s = [n for n in solo if 'k_sweepILi1ELb0ELb0ELb0ELb0ELb%dELi%dELb%dE' % (lrec, fast, box) in n]
                assert len(g) == 1 and len(s) == 1, (lrec, fast, box, sorted(group), sorted(solo))
                vg, vs = _vgprs(group[g[0]][1]), _vgprs(solo[s[0]][1])
                assert vg <= vs, 'k_sweep_group<LREC %d, FAST %d, BOX %d>: %d VGPRs against %d' % (lrec, fast, box, vg, vs)
                assert vg <= 168                                                  # three workgroups of four waves per CU (512 / 3)
                pairs += 1
    assert pairs == 8
