"""Generate tests/golden/k_contribution.npz: the reference's own Visualisation.flux_contribution (Visualisation.py:592-651)
evaluated on the post-step state of step.npz (variant 'lin': positions and modes after the step, occupations after
lifetime_scattering, per-particle temperatures of refresh_temperatures).

    /opt/conda/bin/python3.9 -W ignore tests/golden/make_k_contribution.py

matplotlib runs on Agg; Axes.hist is wrapped to record the `bins` it is given and the histogram `y` it returns for every
connection.  The window-mean temperatures (`mean_T`, read from convergence.txt by the reference) are the step's subvolume
temperatures; the slice filter's inputs (mean_sv_k, std_sv_k, mean_sv_Np) are chosen so that every connection is drawn.
Only data is saved: the inputs handed over and what the reference returned.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

ref = H.import_reference()
from make_golden import material_small  # noqa: E402
import matplotlib.axes  # noqa: E402
import classes.Visualisation as vismod  # noqa: E402
vismod = importlib.reload(vismod)          # import_reference turned flux_contribution into a no-op; this is the original


def main():
    g = np.load(os.path.join(HERE, 'step.npz'))
    p = 'lin__'
    args = H.make_args(ref, H.argv_for('ttp', 20000, 1000))
    geo = ref.Geometry(args)
    ph = H.make_phonon(ref, args, material_small())
    modes = g[p + 'mid_modes'].astype(int)
    q, j = modes[:, 0], modes[:, 1]
    S = geo.n_of_subvols
    mean_T = g[p + 'post_subvol_temperature'].copy()

    v = vismod.Visualisation.__new__(vismod.Visualisation)
    v.args = args
    v.phonon = ph
    v.population = types.SimpleNamespace()
    v.geometry = geo
    v.hbar, v.eVpsa2_in_Wm2, v.a_in_m = ph.hbar, ph.eVpsa2_in_Wm2, ph.a_in_m
    v.q_point, v.branch = q, j
    v.omega = ph.omega[q, j]
    v.velocity = ph.group_vel[q, j, :]
    v.occupation = g[p + 'post_occupation'].copy()
    v.temperatures = g[p + 'post_temperatures'].copy()
    v.subvol_id = g[p + 'post_subvol_id'].copy()
    v.mean_T = mean_T
    v.mean_sv_k, v.std_sv_k, v.mean_sv_Np = np.ones(S), np.zeros(S), np.ones(S)
    v.mean_con_k = np.ones(geo.n_of_subvol_con)
    v.n_of_subvol_con = geo.n_of_subvol_con
    v.folder = args.results_folder

    rec = []
    orig = matplotlib.axes.Axes.hist

    def hist(self, x, *a, **k):
        out = orig(self, x, *a, **k)
        rec.append((np.array(k['bins']), np.array(out[0]), k.get('label', '')))
        return out
    matplotlib.axes.Axes.hist = hist
    try:
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            v.flux_contribution()
    finally:
        matplotlib.axes.Axes.hist = orig

    C = geo.n_of_subvol_con
    assert len(rec) == C, (len(rec), C)
    out = dict(bins=rec[0][0], y=np.array([r[1] for r in rec]), labels=np.array([r[2] for r in rec]),
               subvol_connections=np.asarray(geo.subvol_connections), subvol_con_vectors=np.asarray(geo.subvol_con_vectors),
               mean_T=mean_T, number_of_active_modes=np.array(ph.number_of_active_modes))
    np.savez_compressed(os.path.join(HERE, 'k_contribution.npz'), **out)
    print('k_contribution: %d connections, %d bands, |k| max %.4e' % (C, out['y'].shape[1], np.abs(out['y']).max()))


if __name__ == '__main__':
    main()
