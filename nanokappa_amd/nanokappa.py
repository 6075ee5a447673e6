"""Driver with the flow of the reference's nanokappa.py (:26-107): parameter file -> Geometry -> Phonon ->
Population -> timestep loop -> final state.

    python -m nanokappa_amd.nanokappa -ff parameters.txt
"""
import os
import re
import sys
from datetime import datetime, timedelta

import numpy as np

from .argument_parser import read_args, generate_results_folder
from .geometry import Geometry
from .phonon import Phonon
from .population import Population


def run_replicas(args, geo, phonons, replicas, start, max_time):
    """--replicas R > 1: the time loop of main() for an Ensemble of R populations (seeds seed .. seed + R - 1)."""
    from .ensemble import Ensemble, replica_seeds
    ens = Ensemble(args, geo, phonons, replica_seeds(args.seed, replicas))
    flag = True
    while flag:
        n = min(100 - ens.current_timestep % 100, args.iterations[0] - ens.current_timestep)
        ens.run(max(n, 1))
        flag = (ens.current_timestep < args.iterations[0]) and not ens.finish_sim
        if max_time.total_seconds() > 0:
            flag = flag and datetime.now() - start < max_time
    print('Saving end of run particle data...')
    ens.write_final_state()
    s = ens.write_summary()
    for name in ('kappa', 'con_k'):
        if name in s:
            print('%s over %d replicas: mean %s  std %s  standard error %s' % (name, replicas, s[name]['mean'], s[name]['std'], s[name]['sem']))
    ens.close()
    return ens


def main(argv=None):
    args = read_args(False, argv)
    from .free_path import free_path_option
    fp_n, fp_T, fp_segments = free_path_option(getattr(args, 'free_path', None))     # (refused here, before anything is set up)
    from .free_sweep import sweep_option
    sw_kind, sw_values = sweep_option(getattr(args, 'free_path_sweep', None), fp_n)
    from .free_map import free_path_map_option
    fm_n, fm_kind = free_path_map_option(getattr(args, 'free_path_map', None), fp_n)
    from .kinetic import kinetic_option
    kn_n, kn_T, kn_events = kinetic_option(getattr(args, 'kinetic', None))
    from .kinetic_groups import kinetic_groups_option, BATCHES_DEFAULT
    kg_G, kg_kind, kg_axis = kinetic_groups_option(getattr(args, 'kinetic_groups', None), kn_n)
    from .kinetic_map import kinetic_map_option
    km_n, km_volume = kinetic_map_option(getattr(args, 'kinetic_map', None), kn_n)
    args = generate_results_folder(args)
    out = None
    # nanokappa.py:34-36 compares the parsed value with 'file'; an explicit `--output file` arrives as the list ['file'] and
    # goes to the screen there (only the default writes output.txt).  Fixed here: both spellings write the file.
    mode = args.output[0] if isinstance(args.output, (list, tuple)) else args.output
    if mode == 'file':
        out = open(os.path.join(args.results_folder, 'output.txt'), 'a')
        sys.stdout = out
    with open(os.path.join(args.results_folder, 'arguments.txt'), 'w') as f:   # nanokappa.py:38-50
        for key, val in vars(args).items():
            if isinstance(val, bool):              # a switch (--field_solid): the bare option when on, no line when off
                if val:
                    f.write('--%s\n' % key)
                continue
            f.write('--%s %s\n' % (key, val if isinstance(val, str) else ' '.join(str(i) for i in val)))
    mt = [int(i) for i in re.split('-|:', args.max_sim_time[0])]
    max_time = timedelta(days=mt[0], hours=mt[1], minutes=mt[2], seconds=mt[3])
    start = datetime.now()
    print('Simulation name: %s' % args.results_folder)
    geo = Geometry(args)
    phonons = Phonon(args, 0)
    replicas = int(getattr(args, 'replicas', [1])[0])
    if replicas < 1:
        raise SystemExit('--replicas must be at least 1')
    if replicas > 1:
        ens = run_replicas(args, geo, phonons, replicas, start, max_time)
        print('Total time: %s' % (datetime.now() - start))
        if out is not None:
            sys.stdout = sys.__stdout__
            out.close()
        return ens
    pop = Population(args, geo, phonons)
    if kn_n > 0:                               # --kinetic N [T] [max_events]: after the set-up, before the first step
        print('Kinetic flights: %d rays per reservoir...' % kn_n)
        if kg_G > 0:                           # --kinetic_groups G kind [axis]: the same flights in batches, tallied by group
            kn = pop.kinetic_flights(n=kn_n, T=kn_T, max_events=kn_events, groups=(kg_G, kg_kind, kg_axis), batches=BATCHES_DEFAULT)
        elif km_n is None:
            kn = pop.kinetic_flights(n=kn_n, T=kn_T, max_events=kn_events)
        km = None
        if km_n is not None:                   # --kinetic_map nx ny nz [cell|solid]: the same batches under the same seeds, binned by cell
            km = pop.kinetic_map(km_n, n=kn_n, T=kn_T, max_events=kn_events, batches=BATCHES_DEFAULT, volume=km_volume, kinetic_files=kg_G <= 0)
            if kg_G <= 0:                      # (with groups the grouped flights wrote k_kinetic.txt: rows and sub are the same bits)
                kn = km['summary'] if km is not None else None
        if kn is not None:
            print('  T = %.2f K: %d sources, %d events, %d casts; %d lost, %d missed, %d cut off' %
                  (kn['T'], len(kn['g']), kn['events'].sum(), kn['casts'].sum(), kn['lost'].sum(), kn['missed'].sum(), kn['capped'].sum()))
            if np.isfinite(kn['kappa_eff']):
                print('  kappa_eff = %.4f +- %.4f W/m K over L = %g A (bulk %.4f, free-path closed form %.4f W/m K)' %
                      (kn['kappa_eff'], kn['kappa_eff_se'], kn['L'], kn['kappa_bulk'], kn['kappa_free_path']))
            if kg_G > 0:
                kg = pop.kinetic_groups_last
                print('  %d %s groups in %d batches: kappa from the heat flux = %.4f +- %.4f W/m K; per group %s' %
                      (kg['G'], kg_kind, kg['batches'], float(kg['kappa_flux']), float(kg['kappa_flux_se']),
                       ' '.join('%.4f' % x for x in kg['kappa_g'][:kg['G']])))
            if km is not None:
                se = km['T_se'][np.isfinite(km['T_se'])]
                print('  map of %d x %d x %d cells (%s volume) in %d batches: T from %.3f to %.3f K, largest standard error %.4f K; %d points clamped' %
                      (km['n'] + (km['volume'], km['batches'], np.nanmin(km['T']), np.nanmax(km['T']), se.max() if se.size else np.nan,
                                  int(km['clamped'].sum()))))
    if fp_n > 0:                               # --free_path N [T] [max_segments]: after the set-up, before the first step
        print('Free-path sampling: %d rays per mode...' % fp_n)
        fp = pop.free_paths(n=fp_n, T=fp_T, max_segments=fp_segments)
        if fp is not None:
            a = fp['axis']
            print('  T = %.2f K: kappa_%s%s = %.4f +- %.4f W/m K (an estimate), bulk %.4f W/m K; %d rays missed, %d cut off' %
                  (fp['T'], 'xyz'[a], 'xyz'[a], fp['kappa'][a, a], fp['kappa_se'][a, a], fp['kappa_bulk'][a, a], fp['missed'], fp['capped']))
        if sw_kind is not None:                # --free_path_sweep: the same rays, weighed once per value
            sw = pop.free_path_sweep(sw_kind, sw_values, n=fp_n, T=fp_T, max_segments=fp_segments)
            if sw is not None:
                a = sw['axis']
                print('  sweep over %s, %d casts for %d columns:' % (sw_kind, sw['report']['casts_shared'], len(sw['columns'])))
                for c in sw['columns']:
                    print('    %s %g: kappa_%s%s = %.4f +- %.4f W/m K, bulk %.4f W/m K' %
                          (sw_kind, c['value'], 'xyz'[a], 'xyz'[a], c['kappa'][a, a], c['kappa_se'][a, a], c['kappa_bulk'][a, a]))
        if fm_n is not None:                   # --free_path_map: the same rays, binned by their start cell
            fm = pop.free_path_map(fm_n, n=fp_n, T=fp_T, max_segments=fp_segments, normalise=fm_kind)
            if fm is not None:
                a = fm['axis']
                sup = fm['suppression'][np.isfinite(fm['suppression'])]
                print('  map on %d x %d x %d cells (%s): kappa_%s%s / bulk from %.4f to %.4f over the cells; %d start points clamped' %
                      (fm['n'] + (fm_kind, 'xyz'[a], 'xyz'[a], sup.min() if sup.size else np.nan, sup.max() if sup.size else np.nan,
                                  fm['report']['clamped'])))
    flag = True
    while flag:
        # batches end on the 100-step bookkeeping boundary, so stop criteria are checked as often as the
        # reference's residue is updated
        n = min(100 - pop.current_timestep % 100, args.iterations[0] - pop.current_timestep)
        pop.run(max(n, 1), geo, phonons)
        flag = (pop.current_timestep < args.iterations[0]) and not pop.finish_sim
        if max_time.total_seconds() > 0:
            flag = flag and datetime.now() - start < max_time
    print('Saving end of run particle data...')
    pop.finish_run(geo)
    total = datetime.now() - start
    print('Total time: %s' % total)
    if out is not None:
        sys.stdout = sys.__stdout__
        out.close()
    return pop


if __name__ == '__main__':
    main()
