"""What the multi-step (n-step) return tests share: the synthetic trajectory of tests/test_nstep_cpu.py and tests/test_nstep.py, its ring as the push
kernels write it, and the n-step returns computed the textbook way from per-env episode lists.  Plain functions, nothing heavy at import time.

The trajectory: N = 3 envs.  Env 0 has episodes of length 2 (terminated), 5 (truncated), 1 (terminated), and so on in that cycle; env 1 is never
done; env 2 is done on every step (terminated on even steps, truncated on odd ones).  The reward of env e at push p is 0.1 (p + 1) + 0.01 e."""
import numpy as np

N_ENVS = 3
GAMMA = 0.9
CYCLE = ((2, "term"), (5, "trunc"), (1, "term"))


def step_flags(p):
    """(terminated [3], truncated [3]) of push ``p``."""
    term, trunc = np.zeros(N_ENVS, dtype=bool), np.zeros(N_ENVS, dtype=bool)
    q, c = p, 0
    while q >= CYCLE[c % 3][0]:
        q -= CYCLE[c % 3][0]
        c += 1
    length, how = CYCLE[c % 3]
    if q == length - 1:
        (term if how == "term" else trunc)[0] = True
    (term if p % 2 == 0 else trunc)[2] = True
    return term, trunc


def step_reward(p):
    return 0.1 * (p + 1) + 0.01 * np.arange(N_ENVS)


def ring_host(pushes, capacity, done_column=True):
    """(rows [capacity][68] float32 with reward, mask and -- ``done_column`` -- done filled in, cursor, fill) after ``pushes`` pushes."""
    rows = np.zeros((capacity, 68), dtype=np.float32)
    for p in range(pushes):
        term, trunc = step_flags(p)
        for e in range(N_ENVS):
            r = rows[(p * N_ENVS + e) % capacity]
            r[:] = 0
            r[64], r[65] = np.float32(step_reward(p)[e]), 0.0 if term[e] else 1.0
            if done_column:
                r[67] = 1.0 if term[e] or trunc[e] else 0.0
    total = pushes * N_ENVS
    return rows, total % capacity, min(total, capacity)


def textbook(pushes, capacity, n, gamma=GAMMA):
    """ring row -> (R float32, disc float32, last ring row, m, why) for every live row, from per-env episode lists and not from the ring: the
    transition of env e at push p is live iff p N + e >= total - capacity; its return runs over the following steps of ITS episode, at most n of
    them, and over no step that was not pushed yet.  ``why``: "term", "trunc", "full" or "newest"."""
    episodes = {e: [] for e in range(N_ENVS)}                       # env -> list of episodes, each a list of (push, reward float32, term, trunc)
    open_ep = {e: [] for e in range(N_ENVS)}
    for p in range(pushes):
        term, trunc = step_flags(p)
        for e in range(N_ENVS):
            open_ep[e].append((p, np.float32(step_reward(p)[e]), bool(term[e]), bool(trunc[e])))
            if term[e] or trunc[e]:
                episodes[e].append(open_ep[e])
                open_ep[e] = []
    for e in range(N_ENVS):
        if open_ep[e]:
            episodes[e].append(open_ep[e])
    total, g = pushes * N_ENVS, float(np.float32(gamma))
    out = {}
    for e in range(N_ENVS):
        for ep in episodes[e]:
            for j, (p, _, _, _) in enumerate(ep):
                if p * N_ENVS + e < total - capacity:
                    continue                                        # overwritten
                steps = ep[j:j + n]
                R, disc = 0.0, 1.0
                for k, (_, r, _, _) in enumerate(steps):
                    R = disc * float(r) if k == 0 else R + disc * float(r)
                    disc = disc * g
                pl, _, term, trunc = steps[-1]
                why = "term" if term else "trunc" if trunc else "full" if len(steps) == n else "newest"
                if term and len(steps) == n or trunc and len(steps) == n:
                    why = "term" if term else "trunc"
                out[(p * N_ENVS + e) % capacity] = (np.float32(R), np.float32(disc), (pl * N_ENVS + e) % capacity, len(steps), why)
    return out


def wraps(row, last, capacity):
    """Does the window from ring row ``row`` to ``last`` cross the ring's end?"""
    return last < row
