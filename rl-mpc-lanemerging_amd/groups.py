"""What every group axis shares (traffic, controller, solver and reward groups, populations of members): the checks that ``n`` environments
split into equal groups and that two axes of one run coincide, the per-group ``summary``, and the splitmix64 finaliser behind the groups' seeds.
The callers give the nouns and the limits, so every message reads as the axis that raises it worded it.  Touches no device."""
_M64 = 0xFFFFFFFFFFFFFFFF


def within(count, limit, what, unit="groups"):
    """``count`` if ``what`` names 1 ... ``limit`` ``unit``; ValueError otherwise."""
    if not 1 <= count <= limit:
        raise ValueError("%s must name 1 ... %d %s, not %d" % (what, limit, unit, count))
    return count


def split(n, count, limit, what, noun=None):
    """(count, n_per_group) for ``n`` environments in ``count`` groups of the axis ``what`` (its groups are "``noun`` groups", default ``what``);
    ValueError unless there are 1 ... ``limit`` groups and ``n`` splits into them equally."""
    within(count, limit, what)
    if int(n) < count or int(n) % count:
        raise ValueError("n = %d environments do not split into %d %s groups of equal size" % (n, count, noun or what))
    return count, int(n) // count


def coincide(what, count, n_per_group, traffic=None, policy=None):
    """Cell c of a run pairs group c of every axis: ValueError unless the ``count`` groups of ``n_per_group`` environments of the axis ``what``
    coincide with the traffic groups ``traffic`` (a list or None) and with the members of ``policy`` (checked if it is a population: has ``P``)."""
    if traffic is not None and len(traffic) != count:
        raise ValueError("the traffic has %d groups, the %s %d: cell c pairs traffic c with %s c, so they must coincide" % (len(traffic), what, count, what))
    if hasattr(policy, "P") and (policy.P != count or policy.n_per_member != n_per_group):
        raise ValueError("the population has %d members of %d environments, the %s %d groups of %d: cell c pairs member c with %s c, so they must coincide"
                         % (policy.P, policy.n_per_member, what, count, n_per_group, what))


def summary_by(stats, count, what):
    """``episodes.summary`` of each part's environments: ``count`` dicts, part p from rows [p * n / count, (p + 1) * n / count) of every column
    of a run's result; ``what``: the parts' plural noun ("members", "traffic groups", ...)."""
    from .episodes import summary
    n = len(stats["status"])
    if count < 1 or n % count:
        raise ValueError("%d environments do not split into %d %s" % (n, count, what))
    per = n // count
    return [summary({k: v[p * per:(p + 1) * per] for k, v in stats.items() if k != "report"}) for p in range(count)]


def splitmix64(z):
    """The finaliser of splitmix64 on the Python int ``z`` (taken below 2**64): the mixing step of ``stmpc_env_episode_seed``, the traffic mix's
    draw and the learner's generator."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)
