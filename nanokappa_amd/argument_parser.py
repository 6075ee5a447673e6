"""Parameter-file / command-line front end with the reference's flags and semantics
(reference argument_parser.py:6-181): `--from_file <txt>` splits the file on whitespace and feeds argparse.
Additions: `--seed` (the reference uses the unseeded global NumPy generator), `--device`, `--spectral_bands`, `--field_grid`, `--field_groups`, `--field_solid`, `--mode_tally`, `--free_path`, `--free_path_sweep`, `--free_path_map`, `--kinetic`, `--kinetic_groups` and `--kinetic_map`."""
import argparse
import os
import sys


def initialise_parser(debug_flag=False):
    p = argparse.ArgumentParser()
    a = p.add_argument
    a('--from_file', '-ff', default='', type=str, nargs=1)
    a('--geometry', '-g', default=['cuboid'], type=str, nargs=1)
    a('--dimensions', '-d', default=[10e3, 1e3, 1e3], type=float, nargs='*')
    a('--scale', '-s', default=[1, 1, 1], type=float, nargs=3)
    a('--geo_rotation', '-gr', default=[0, 0, 0, 'xyz'], nargs='*')
    a('--mat_rotation', '-mr', default=[], nargs='*')
    a('--isotope_scat', '-is', default=[], type=int, nargs='*')
    a('--particles', '-p', default=['pmps', 1], nargs=2)
    a('--timestep', '-ts', default=[1], type=float, nargs=1)
    a('--iterations', '-i', default=[10000], type=int, nargs=1)
    a('--max_sim_time', '-mt', default=['1-00:00:00'], type=str, nargs=1)
    a('--subvolumes', '-sv', default=[], nargs='*')
    a('--temp_dist', '-td', default=['cold'], choices=['cold', 'hot', 'linear', 'mean', 'random', 'custom'], type=str, nargs='*')
    a('--temp_interp', '-ti', default=['nearest'], choices=['nearest', 'linear', 'radial'], type=str, nargs=1)
    a('--subvol_temp', '-st', default=[], type=float, nargs='*')
    a('--bound_cond', '-bc', default=[], choices=['T', 'P', 'R'], type=str, nargs='*')
    a('--bound_pos', '-bp', default=[], nargs='*')
    a('--bound_values', '-bv', default=[], type=float, nargs='*')
    a('--connect_pos', '-cp', default=[], nargs='*')
    a('--fig_plot', '-fp', default=[], type=str, nargs='*')
    a('--colormap', '-cm', default=['jet'], type=str, nargs=1)
    a('--theme', '-th', default=['white'], choices=['white', 'light', 'dark'], type=str, nargs=1)
    a('--n_mean', '-nm', default=[100], type=int, nargs=1)
    a('--conv_crit', '-cc', default=[0, 1], type=float, nargs=2)
    a('--mat_folder', '-mf', default=[''], type=str, nargs='*')
    a('--poscar_file', '-pf', required=True, type=str, nargs='*')
    a('--hdf_file', '-hf', required=True, type=str, nargs='*')
    a('--results_folder', '-rf', default=[], type=str, nargs='*')
    a('--part_dist', '-pd', default=['random_subvol'], type=str, nargs=1)
    a('--empty_subvols', '-es', default=[], type=int, nargs='*')
    a('--subvol_material', '-sm', default=[], type=int, nargs='*')
    a('--reference_temp', '-rt', default=['local'], nargs=1)
    a('--reservoir_gen', '-gn', default=['constant'], choices=['fixed_rate', 'one_to_one', 'constant'], type=str, nargs='*')
    a('--path_points', '-pp', default=[], nargs='*')
    a('--energy_normal', '-en', default=['mean'], type=str, nargs=1)
    a('--bound_scat', '-bs', default=['velocity'], type=str, nargs='*')
    a('--output', '-op', default='file', type=str, nargs=1)
    # additions of this build
    a('--seed', default=[0], type=int, nargs=1, help='seed of the counter-based RNG (Philox4x32-10)')
    a('--device', default=[0], type=int, nargs=1, help='HIP device index')
    a('--spectral_bands', default=['0', 'frequency'], type=str, nargs='*',
      help='N [frequency|branch] (or just: branch): tally the heat flux in N frequency bands, or one band per branch, on '
           'every heat-flux step and write the frequency-resolved conductivity to k_contribution.txt; 0 = off')
    a('--field_grid', default=[], type=str, nargs='*',
      help='nx ny nz [every]: sum particle count, energy and heat flux on a uniform grid of nx x ny x nz cells over the '
           'bounding box every `every` steps (default 100, a multiple of 10) on the GPU, averaged over the convergence '
           'window, and write field.vtk; the counterpart of the particle scatter of --fig_plot; off by default')
    a('--field_groups', default=[], type=str, nargs='*',
      help='G kind [axis]: with --field_grid, also sum count, energy and heat flux per (cell, group of modes) on the GPU and '
           'write field_groups.npz; kind = frequency (G bins), branch (one group per branch), mfp (G log-spaced bins of the '
           'mean free path at the mean reservoir temperature) or direction (G bins of the cosine between the group velocity '
           'and the axis x|y|z, default the slice axis); off by default')
    a('--field_solid', action='store_true', default=False,
      help='with --field_grid: compute the exact solid fraction of every grid cell on the GPU, once; --energy_normal fixed '
           'then divides by the volume of solid in a cell instead of the whole cell (cells cut by the surface read right), '
           'and field.vtk / field_groups.npz carry solid_fraction; off by default')
    a('--mode_tally', default=['0'], type=str, nargs='*',
      help='[every]: tally energy and particle count per (subvolume, mode) every `every` steps (default 100, a multiple of '
           'n_dt_to_conv = 10) on the GPU over the convergence window, and write mode_tally.npz and the conductivity '
           'accumulated over the mean free path, k_accumulation.txt; 0 = off (the default)')
    a('--free_path', default=[], type=str, nargs='*',
      help='N [T] [max_segments]: before the first step, estimate the conductivity the geometry and the material alone allow by '
           'free-path sampling on the GPU -- N rays per mode from start points uniform in the solid, flown along the group '
           'velocity until a boundary ends them, weighed with the lifetimes at T (default: the mean reservoir temperature) -- '
           'and write k_free_path.txt (tensor with its standard error, bulk value, accumulation over the mean free path) and '
           'free_path.npz (per-mode arrays); off by default')
    a('--kinetic', default=[], type=str, nargs='*',
      help='N [T] [max_events]: before the first step, solve the steady linearised BTE (relaxation time) by kinetic flights on the '
           'GPU -- N energy packets from every reservoir (T facet), flown, scattered with the lifetimes at T (default: the mean '
           'reservoir temperature), re-emitted by diffuse walls and absorbed by reservoirs -- and write k_kinetic.txt (conductance '
           'between the reservoirs with its standard error, kappa_eff between two parallel reservoirs, the bulk value) and '
           'kinetic.npz (transmission, temperature deviation and heat flux per subvolume); off by default')
    a('--kinetic_groups', default=[], type=str, nargs='*',
      help='G kind [axis]: with --kinetic N, also tally the flights\' dwell time and heat flux per (subvolume, group of modes) on '
           'the GPU, in 8 batches of N / 8 rays whose spread gives the error bars, and write k_kinetic_groups.txt (one line per '
           'group: its edges, its share of the conductivity between the reservoirs with its standard error, the bulk share, their '
           'ratio, the running sum -- the accumulation function with the contacts included) and kinetic_groups.npz (per group the '
           'temperature deviation and heat flux of every subvolume); kind = frequency (G bins), branch, mfp (G log-spaced bins of '
           'the mean free path of the call\'s lifetimes) or direction (G bins of the cosine between the group velocity and the '
           'axis x|y|z, default the transport axis); off by default')
    a('--kinetic_map', default=[], type=str, nargs='*',
      help='nx ny nz [cell|solid]: with --kinetic N, also bin every segment of the flights on the GPU into the cells of an nx x ny '
           'x nz grid over the bounding box (the grid of --field_grid), in 8 batches of N / 8 rays whose spread gives the error '
           'bars, and write kinetic_map.npz and kinetic_map.vtk -- the steady temperature T, its deviation dT and the heat flux q '
           'of every cell with their standard errors; cell (the default) divides by the cell volume, solid by the exact solid '
           'volume of every cell (and adds solid_fraction); off by default')
    a('--free_path_sweep', default=[], type=str, nargs='*',
      help='scale s1 s2 ... | temperature T1 T2 ...: with --free_path N, also weigh the same rays once per value (at most 32) -- '
           'the structure scaled by s with unchanged roughness, or the structure as it is at the temperature T (K) -- and write '
           'k_free_path_sweep.txt (one line per value: kappa along the axis, its standard error, the bulk value, their ratio) and '
           'free_path_sweep.npz (per value the tensors, the per-mode suppression, the accumulation over the mean free path on '
           'one grid); off by default')
    a('--free_path_map', default=[], type=str, nargs='*',
      help='nx ny nz [count|solid]: with --free_path N, also bin the same rays on the GPU by the cell of their start point on a '
           'grid of nx x ny x nz cells over the bounding box (the grid of --field_grid) and write free_path_map.npz and '
           'free_path_map.vtk: the local conductivity tensor per cell, its ratio to the bulk value along the axis, the rays per '
           'cell and how they ended -- where the walls cut the heat flow, before a step is run (an estimate); count divides by '
           'the rays a cell received (the default), solid by the exact volume of solid in it; off by default')
    a('--replicas', default=[1], type=int, nargs=1,
      help='R: run the same problem under the seeds seed, seed + 1, ..., seed + R - 1 (an error bar on the conductivity); '
           'every replica writes its files to replica_<k> of the results folder, ensemble.txt holds the mean, the standard '
           'deviation and the standard error over the replicas; where the configuration allows, all replicas advance by '
           'shared GPU launches; 1 = a single run (the default)')
    return p


def read_args(debug_flag=False, argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if '-ff' in argv or '--from_file' in argv:
        key = '-ff' if '-ff' in argv else '--from_file'
        filename = argv[argv.index(key) + 1]
        with open(filename, 'r') as f:
            args = initialise_parser(debug_flag).parse_args(f.read().split())
        args.from_file = filename
        return args
    return initialise_parser(debug_flag).parse_args(argv)


def get_folder_index(loc):
    base, dirname = os.path.basename(loc), os.path.dirname(loc)
    if not os.path.exists(dirname):
        return 0
    same = []
    for d in os.listdir(dirname):
        if base in d:
            try:
                same.append(int(d.split('_')[-1]))
            except ValueError:
                pass
    return max(same) + 1 if same else 0


def generate_results_folder(args):
    if len(args.results_folder) == 0:
        args.results_folder = os.getcwd()
        return args
    loc = os.path.normpath(os.path.relpath(args.results_folder[0]))
    if not os.path.isabs(loc):
        loc = os.path.join(os.getcwd(), loc)
    i = get_folder_index(loc)
    os.makedirs('%s_%d' % (loc, i), exist_ok=False)
    args.results_folder = '%s_%d' % (loc, i)
    return args
