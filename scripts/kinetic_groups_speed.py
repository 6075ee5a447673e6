"""Speed of the grouped kinetic flights (k_kinetic<.., true> + k_kinetic_fold, nk_kinetic_flights_groups) beside the plain call
(k_kinetic<.., false>, nk_kinetic_flights) on the same geometry in the same process, by the protocol of scripts/kinetic_speed.py:
BASELINE config 2's material and box and the 72-sided wire, the lifetimes at 300 K and a sixteenth of them, N = 2^20 rays per
source, legs alternated, five repeats after one warm-up call each, medians and ranges of the reports' `seconds` (HIP events
around the launches).  The legs: the plain call; 'mfp' with 16 groups (columns in LDS bins); 'frequency' with as many groups as
push the columns out of LDS (straight to memory); and, with --other-lib, the plain call of another build of the library (the
parent commit's, to see that the plain instantiations still run at their speed).  On config 2 it also prints kappa per group,
suppression and accumulation over the mean free path from 8 batches, beside the free-path pass's shares in the same groups.

    python scripts/kinetic_groups_speed.py [--reps 5] [--n 1048576] [--cases c2 wire72] [--other-lib PATH] [--result-n 4194304]
                                           [--out profiles/kinetic_groups_notes.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from free_sweep_speed import engine_c2, engine_wire72, spread  # noqa: E402


def other_engine(case, path, optional=('nk_kinetic_flights_groups', 'nk_kinetic_flights_map')):
    """The case's engine on another build of the library (engine.load_library(path); the entries named in `optional` may be missing
    there: only the plain call is made on it).  The set-up is engine_c2's / engine_wire72's with that engine."""
    from nanokappa_amd.engine import Engine, load_library
    lib = load_library(path, optional=optional)
    if case == 'c2':
        import bench
        from nanokappa_amd import synthetic
        from nanokappa_amd.argument_parser import initialise_parser
        from nanokappa_amd.geometry import Geometry
        from nanokappa_amd.phonon import Phonon
        from nanokappa_amd.population import Population
        argv, species, _ = bench.config_argv('c2', 100000, 200.0)
        args = initialise_parser().parse_args(argv + ['--seed', '2025', '--device', '0'])
        args.results_folder = ''
        geo = bench.quiet(Geometry, args)
        ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
        pop = bench.quiet(Population, args, geo, ph, engine=Engine(0, 2025, library=lib))
        return pop.engine, pop
    import free_path_cases as FC
    ct = FC.case('wire72')
    eng = Engine(0, 5, library=lib)
    eng.set_material(ct['tables'])
    eng.set_mesh(ct['mesh'])
    S = ct['centers'].shape[0]
    eng.set_subvolumes(ct['centers'], ct['volumes'], ct.get('kind', 0), ct['axis'], 1 if ct.get('kind', 0) == 0 else 2, np.full(S, 300.0))
    r = ct['rough']
    eng.set_rough(r['facets'], r['specularity'], r['true_spec'], r['spec_map'], r['roulette'], degen_j2=r.get('degen_j2'))
    return eng, ct


def spill_groups(nsrc, S):
    """The smallest power of two G whose nsrc x S x (G + 1) x 4 words cannot fit in 64 KB of LDS."""
    G = 2
    while nsrc * S * (G + 1) * 32 <= 64 * 1024 and G < 256:
        G *= 2
    return G


def measure(name, eng, other, ph, tau, c, n, reps, lines):
    from nanokappa_amd import kinetic_groups as KG
    for label, scale in (('tau', 1.0), ('tau/16', 1.0 / 16.0)):
        t = np.where(tau > 0, tau * scale, tau)
        warm = eng.kinetic_flights(t, c, n=64)
        S = warm['sub'].shape[1]
        tm, _, _ = KG.build('mfp', 16, ph, t, eng._vg)
        Gs = spill_groups(warm['sub'].shape[0], S)
        tf, _, _ = KG.build('frequency', Gs, ph, t, eng._vg)
        legs = [('plain', eng, None), ('mfp G = 16', eng, (16, tm)), ('frequency G = %d' % Gs, eng, (Gs, tf))]
        if other is not None:
            legs.insert(1, ('plain, other library', other, None))
        call = lambda e, g: e.kinetic_flights(t, c, n=n) if g is None else e.kinetic_flights(t, c, n=n, groups=g)
        res = {k: [] for k, _, _ in legs}
        last = {}
        for k, e, g in legs:                                          # warm-up of every leg
            call(e, g)
        for _ in range(reps):
            for k, e, g in legs:
                last[k] = call(e, g)
                res[k].append(last[k]['report'])
        p = res['plain'][0]
        lines.append('%-7s %-7s geometry mode %d  %d rays, %.4g events, %d subvolumes, grid %d' % (name, label, p['geometry_mode'], p['rays'], p['events'], S, p['grid']))
        for k, _, g in legs:
            r = res[k]
            same = np.array_equal(last[k]['sub'], last['plain']['sub']) and np.array_equal(last[k]['rows'], last['plain']['rows'])
            cols = '' if g is None else '; columns sum to sub: %s' % np.array_equal(last[k]['grp'].sum(axis=2), last[k]['sub'])
            lines.append('          %-22s %s ms   lds bins %d; sub and rows equal to the plain call\'s: %s%s'
                         % (k, spread([x['seconds'] for x in r]), r[0]['lds_bins'], same, cols))
        print('\n'.join(lines[-len(legs) - 1:]), flush=True)


def config2(pop, n, lines):
    s = pop.kinetic_flights(n=n, groups=(16, 'mfp'), batches=8, write=False)
    g = pop.kinetic_groups_last
    lines.append('config 2: T = %.1f K, N = %d per source in %d batches, 16 mfp groups: kappa_eff (counts) = %.4f +- %.4f, kappa_flux = %.4f +- %.4f W/m K (bulk %.2f)'
                 % (s['T'], s['n'], g['batches'], s['kappa_eff'], s['kappa_eff_se'], float(g['kappa_flux']), float(g['kappa_flux_se']), s['kappa_bulk']))
    lines.append('          mfp from (A)   to (A)        kappa_g      se         kappa_bulk_g  suppression  accumulated  (W/m K)')
    for i in range(g['G']):
        lines.append('          %-12.5g   %-12.5g  %-11.5f  %-9.5f  %-12.5f  %-11.5f  %-.5f' % (g['edges'][i], g['edges'][i + 1], g['kappa_g'][i], g['kappa_g_se'][i],
                                                                                           g['kappa_bulk_g'][i], g['suppression'][i], g['accumulation'][i]))
    lines.append('          rest column (live modes that do not move): kappa %.3g; dT_g at the hot and the cold end per group (K):' % g['kappa_g'][g['G']])
    lines.append('          ' + ' '.join('%+.3f' % x for x in g['dT_g'][0, :g['G']]))
    lines.append('          ' + ' '.join('%+.3f' % x for x in g['dT_g'][-1, :g['G']]))
    lines.append('          standard errors of the hot end\'s, from the batches: ' + ' '.join('%.3f' % x for x in g['dT_g_se'][0, :g['G']]))
    col = g['table'][g['table'] >= 0]
    lines.append('          modes per group: ' + ' '.join('%d' % x for x in np.bincount(col, minlength=g['G'])) + '; c_g / sum c: ' +
                 ' '.join('%.2e' % x for x in g['c_g'][:g['G']] / g['c_g'].sum()))
    print('\n'.join(lines[-(g['G'] + 7):]), flush=True)
    return g


def beside(pop, g, lines):
    """Config 2's kappa per mfp group from the kinetic flights beside the free-path pass's (Population.free_paths, 64 rays per mode,
    its per-mode shares along the axis binned by the same table), with the running sums."""
    from nanokappa_amd import kinetic_groups as KG
    G = g['G']
    col = KG.columns(g['table'], G)
    fp = pop.free_paths(n=64, write=False)
    k_fp = np.bincount(col[fp['modes']], weights=fp['k_mode'], minlength=G + 1)
    lines.append('          kappa per mfp group (W/m K): kinetic flights | free-path pass (64 rays per mode), then the running sums')
    cols = [g['kappa_g'], k_fp]
    for i in range(G):
        lines.append('          %-12.5g %-12.5g  ' % (g['edges'][i], g['edges'][i + 1]) + '  '.join('%9.5f' % c[i] for c in cols) + '   |  ' +
                     '  '.join('%9.5f' % c[:i + 1].sum() for c in cols))
    lines.append('          rest column: ' + '  '.join('%9.5f' % c[G] for c in cols))
    print('\n'.join(lines[-(G + 2):]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--cases', nargs='*', default=['c2', 'wire72'])
    ap.add_argument('--other-lib', default='')
    ap.add_argument('--result-n', type=int, default=0, help='also print config 2\'s kappa per mfp group at so many rays per source')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    from nanokappa_amd import kinetic as KN
    lines = ['device milliseconds: median (min .. max) of %d repeats, legs alternated, after one warm-up call each; N = %d rays per source' % (a.reps, a.n)]
    if a.other_lib:
        lines.append('other library: %s' % os.path.basename(a.other_lib))
    for case in a.cases:
        make = engine_c2 if case == 'c2' else engine_wire72
        eng, tau, keep = make()
        other, okeep = None, None
        if a.other_lib:
            other, okeep = other_engine(case, os.path.abspath(a.other_lib))
        if case == 'c2':
            ph = keep._ph
            c = KN.heat_capacity(ph.omega, 300.0, ph.number_of_qpoints * ph.volume_unitcell, keep.hbar, keep.kb)
            measure(case, eng, other, ph, tau, c, a.n, a.reps, lines)
            if a.result_n > 0:
                g = config2(keep, a.result_n, lines)
                beside(keep, g, lines)
        else:
            import kinetic_cases as K
            measure(case, eng, other, keep['ph'], tau, K.heat_capacity(keep), a.n, a.reps, lines)
        eng.close()
        if other is not None:
            other.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
