"""Test-side restatement of the reward map (include/aac_rmap.h): ``ss_reward`` of the subject alone at a
test position, everything else the env's state as it stands.  Built on tests/terms_ref.py (the oracles are
imported, not edited): on a deep copy of an ``AttTerms`` / ``WgruTerms`` env the subject's ``pos`` and
``pre_pos`` are set (ATT/env:2133-2138, WGRU/env:1687-1692), ``ss_reward_terms`` runs, and the subject's
row is taken.  The input env is left untouched, so every point sees the same state -- the map's read-only
rule -- and the WGRU +3 waypoint bonus stays in (slot 1 is what a step would earn).

WGRU radar minimum: a given ``rmin`` is used verbatim; with None the obstacle radar is taken at the point
itself (``WgruTerms.radar``), the value a step landing there ends up with.  No GPU needed."""
import copy

import numpy as np

from tests import terms_ref as R


def row(env, agent, point, pre=None, rmin=None):
    """(terms (12,), own reward, done, mask, bbc (4,)) of ``agent`` of ``env`` standing at ``point`` with
    ``pre_pos = pre`` (None: the point).  ``env`` itself is not changed."""
    env = copy.deepcopy(env)
    ag = env.all_agents[agent]
    ag.pos = np.array([float(point[0]), float(point[1])])
    ag.pre_pos = ag.pos.copy() if pre is None else np.array([float(pre[0]), float(pre[1])])
    env.get_current_agent_nei(ag)
    for other in env.all_agents.values():          # the other rows are computed and dropped: they only need
        if not other.surroundingNeighbor:          # their loops' inputs in place
            env.get_current_agent_nei(other)
    wgru = isinstance(env, R.WgruTerms)
    if wgru:
        for i, other in env.all_agents.items():
            if i == agent or len(np.atleast_1d(other.observableSpace)) == 0:
                other.observableSpace = env.radar(i)
        rm = None
        if rmin is not None:
            rm = [float(rmin) if i == agent else float(np.min(env.all_agents[i].observableSpace))
                  for i in range(env.N)]
        terms, rew, done, masks = env.ss_reward_terms(rm)
    else:
        terms, rew, done, masks = env.ss_reward_terms()
    m, d = int(masks[agent]), bool(done[agent])
    bound = bool(m & 1)
    if wgru:         # [bound, building, 0, 0]: the branch taken (WGRU/env:1956, :1963)
        bbc = [bound, (not bound) and bool(m & 8), False, False]
    else:            # [bound, 0, drone, last contact == nearest] (ATT/env:2490-2530)
        drone = (not bound) and bool(m & 2)
        last_is_nearest = False
        if drone:
            p = env.all_agents[agent].pos
            ds = {k: np.linalg.norm(p - env.all_agents[k].pos) for k in range(env.N) if k != agent}
            nearest = min(ds, key=lambda k: (ds[k], k))       # the first strict minimum in index order
            last = max(k for k, v in ds.items() if v <= 5.0)
            last_is_nearest = last == nearest
        bbc = [bound, False, drone, last_is_nearest]
    return terms[agent].copy(), float(rew[agent]), d, m, np.array(bbc, np.uint8)


def prepare(env):
    """Fill in what ``ss_reward_terms`` reads of every agent (neighbour sets; WGRU: radar rows) on an env
    that has not been stepped yet.  Changes ``env``: for envs this module built itself."""
    for i, ag in env.all_agents.items():
        env.get_current_agent_nei(ag)
        if isinstance(env, R.WgruTerms):
            ag.observableSpace = env.radar(i)
    return env


def rows(variant, st, occ, points, env_idx=None, agent=None, pre=None, rmin=None, mode=0):
    """The map of M points over a tests/thresholds.py (``variant="att"``) or tests/wgru_thresholds.py
    (``"wgru"``) state dict: ``env_idx`` / ``agent`` [M] (None: 0), ``pre`` [M][2] or None, ``rmin`` [M] or
    None.  Returns dict(terms [M][12], reward [M], done [M], mask [M], bbc [M][4])."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    M = points.shape[0]
    env_idx = np.zeros(M, np.int64) if env_idx is None else np.broadcast_to(np.asarray(env_idx), (M,))
    agent = np.zeros(M, np.int64) if agent is None else np.broadcast_to(np.asarray(agent), (M,))
    envs = {}
    out = dict(terms=np.zeros((M, R.WIDTH)), reward=np.zeros(M), done=np.zeros(M, np.uint8),
               mask=np.zeros(M, np.uint8), bbc=np.zeros((M, 4), np.uint8))
    for m in range(M):
        e = int(env_idx[m])
        if e not in envs:
            envs[e] = prepare(R.wgru_env(st, e, occ) if variant == "wgru" else R.att_env(st, e, occ, mode))
        t, r, d, k, b = row(envs[e], int(agent[m]), points[m], None if pre is None else pre[m],
                            None if rmin is None else rmin[m])
        out["terms"][m], out["reward"][m], out["done"][m], out["mask"][m], out["bbc"][m] = t, r, d, k, b
    return out
