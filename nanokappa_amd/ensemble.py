"""The same problem under several seeds: R Populations advanced together, for an error bar on the conductivity.

Where the library can group their engines (engine.EngineGroup / nk_group_create: small meshes without rough facets, generators
'constant' / 'fixed_rate', one rank, no band / field / mode tally) every timestep of all R replicas is ONE sweep launch and ONE tail
launch; where it cannot, the populations are stepped one after another and `why_not` says why.  Either way every replica writes
the files a run of its own would write, into `replica_<k>` of the results folder, and `ensemble.txt` holds the statistics over
the replicas.
"""
import copy
import os

import numpy as np

from .engine import EngineGroup, NkError, ERR_ARG
from .population import Population, _Stats


def replica_seeds(seed, replicas):
    """--seed s --replicas R: seeds s, s + 1, ..., s + R - 1."""
    seed = int(seed[0] if isinstance(seed, (list, tuple)) else seed)
    replicas = int(replicas[0] if isinstance(replicas, (list, tuple)) else replicas)
    if replicas < 1:
        raise ValueError('--replicas must be at least 1')
    return [seed + k for k in range(replicas)]


def replica_folder(results_folder, k, create=True):
    """Results folder of replica k: `replica_<k>` inside the run's folder ('' = no files, like a Population without a folder)."""
    if not results_folder:
        return ''
    path = os.path.join(results_folder, 'replica_%d' % k)
    if create:
        os.makedirs(path, exist_ok=True)
    return path


def replica_args(args, seed, k, create=True):
    """A copy of the parsed arguments for replica k: its own seed and its own results folder."""
    a = copy.copy(args)
    a.seed = [int(seed)]
    a.results_folder = replica_folder(args.results_folder, k, create)
    return a


def replica_statistics(pop):
    """Mean and std over the last n_mean convergence rows of one replica (what _Stats computes): dict name -> (mean, std),
    each an array: kappa [1] (slice subvolumes) or con_k [connections], T_sv [S], phi [3 S]."""
    v = _Stats(pop)
    v.postprocess()
    out = {}
    if pop.subvol_type == 'slice':
        out['kappa'] = (np.atleast_1d(v.mean_k), np.atleast_1d(v.std_k))
    else:
        out['con_k'] = (np.atleast_1d(v.mean_con_k), np.atleast_1d(v.std_con_k))
    out['T_sv'] = (np.atleast_1d(v.mean_T), np.atleast_1d(v.std_T))
    out['phi'] = (np.atleast_1d(v.mean_sv_phi), np.atleast_1d(v.std_sv_phi))
    return out


def across_replicas(values):
    """values [R, n] (one row per replica): mean, sample standard deviation (ddof = 1) and standard error over the replicas."""
    a = np.asarray(values, dtype=float)
    a = a.reshape(a.shape[0], -1)
    R = a.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = a.mean(axis=0)
        std = a.std(axis=0, ddof=1) if R > 1 else np.full(a.shape[1], np.nan)
        sem = std / np.sqrt(R)
    return mean, std, sem


def summarise(per_replica):
    """per_replica: list of replica_statistics dicts -> dict name -> dict(mean, std, sem over the replicas [n]; replica_mean,
    replica_std [R, n])."""
    out = {}
    for name in per_replica[0]:
        rm = np.array([np.ravel(p[name][0]) for p in per_replica], dtype=float)
        rs = np.array([np.ravel(p[name][1]) for p in per_replica], dtype=float)
        mean, std, sem = across_replicas(rm)
        out[name] = dict(mean=mean, std=std, sem=sem, replica_mean=rm, replica_std=rs)
    return out


def write_summary(path, summary, seeds, grouped, why_not):
    """ensemble.txt: one line per scalar -- quantity, index, then mean, std (ddof = 1) and standard error over the replicas, then
    every replica's own mean and std over its convergence window.  Numbers with 17 significant digits (they read back exactly)."""
    with open(path, 'w') as f:
        f.write('# replicas %d  seeds %s\n' % (len(seeds), ' '.join(str(s) for s in seeds)))
        f.write('# grouped %s\n' % ('yes' if grouped else 'no: ' + str(why_not).replace('\n', ' ')))
        f.write('# quantity index mean std sem' + ''.join(' mean_%d std_%d' % (k, k) for k in range(len(seeds))) + '\n')
        for name, q in summary.items():
            for i in range(q['mean'].shape[0]):
                cols = [q['mean'][i], q['std'][i], q['sem'][i]]
                for k in range(len(seeds)):
                    cols += [q['replica_mean'][k, i], q['replica_std'][k, i]]
                f.write('%s %d ' % (name, i) + ' '.join('%.17e' % c for c in cols) + '\n')


def read_summary(path):
    """ensemble.txt back: dict name -> array [n, 3 + 2 R] (mean, std, sem, then mean_k, std_k per replica)."""
    out = {}
    with open(path) as f:
        for line in f:
            if line.startswith('#') or not line.strip():
                continue
            w = line.split()
            out.setdefault(w[0], []).append([float(x) for x in w[2:]])
    return {k: np.array(v) for k, v in out.items()}


class Ensemble(object):
    """R Populations of the same arguments, one per seed, advanced together."""

    def __init__(self, args, geometry, phonon, seeds):
        self.args = args
        self.geometry, self.phonon = geometry, phonon
        self.seeds = [int(s) for s in seeds]
        if not self.seeds:
            raise ValueError('Ensemble: no seeds')
        self.results_folder_name = args.results_folder
        self.populations = []
        for k, s in enumerate(self.seeds):
            print('Replica %d (seed %d)' % (k, s))
            self.populations.append(Population(replica_args(args, s, k), geometry, phonon))
        self.group, self.grouped, self.why_not = None, False, None
        self._retry = False            # grouping ended in mid-run (a store was re-laid out): asked for again every 100 steps
        self._try_group()

    def _try_group(self):
        try:
            self.group = EngineGroup([p.engine for p in self.populations])
            self.grouped, self.why_not = True, None
        except NkError as e:
            self._ungroup(str(e))

    def _ungroup(self, why):
        if self.group is not None:
            self.group.close()
        self.group, self.grouped, self.why_not = None, False, why
        print('Replicas are stepped one after another: %s' % why)

    @property
    def current_timestep(self):
        return self.populations[0].current_timestep

    @property
    def finish_sim(self):
        return all(p.finish_sim for p in self.populations)

    def run(self, nsteps):
        """Advance every replica by nsteps timesteps, with the chunking of Population.run (library calls end on the 100-step
        bookkeeping boundaries): every replica's outputs are those of a run of its own."""
        geo, ph = self.geometry, self.phonon
        for p in self.populations:
            p._begin_run(geo, ph)
        done = 0
        while done < nsteps:
            chunk = min(p._plan_chunk(nsteps - done, geo) for p in self.populations)
            if self.group is None and self._retry and (self.current_timestep % 100) == 0:
                self._try_group()          # the members are still at the same step: they may agree again
                self._retry = self.group is None
            ts = None
            if self.group is not None:
                try:
                    ts = self.group.step(chunk)
                except NkError as e:
                    if getattr(e, 'code', 0) != ERR_ARG:     # NK_ERR_ARG: refused before anything ran (a store was re-laid out, ...)
                        raise
                    self._ungroup(str(e))
                    self._retry = True
            if ts is None:
                ts = [p.engine.step(chunk) for p in self.populations]
            for p, t in zip(self.populations, ts):
                p._consume_chunk(t, chunk, geo, ph)
            done += chunk

    def summary(self):
        """Per replica the mean and std of kappa, T_sv and the heat flux over the last n_mean convergence rows; over the
        replicas the mean, the sample standard deviation and the standard error of those means."""
        return summarise([replica_statistics(p) for p in self.populations])

    def write_summary(self):
        s = self.summary()
        if self.results_folder_name:
            write_summary(os.path.join(self.results_folder_name, 'ensemble.txt'), s, self.seeds, self.grouped, self.why_not)
        return s

    def write_final_state(self):
        """Every replica's end-of-run files, as a run of its own writes them (Population.finish_run): the final state, and
        k_contribution.txt / field.vtk / mode_tally.npz + k_accumulation.txt where those tallies are on."""
        for p in self.populations:
            if p.results_folder_name:
                p.finish_run(self.geometry)
            else:
                p.view.postprocess()

    def close(self):
        if self.group is not None:
            self.group.close()
            self.group = None
