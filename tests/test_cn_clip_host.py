"""The check pass of bp_run (csrc/swd_osdw_kernel.h) clips once per check: the walk keeps the two smallest |x| and `min(., 50)` is
applied to the two minima behind the walk and the quad merges, instead of to every position in front of the two-minimum update.
Clipping is monotone, so it commutes with the order statistics; the position named as "first minimum" may differ only where the
clipped minima tie at 50, and there both stored magnitudes are the same.

This file restates one check's read / merge / write in plain Python doubles, both ways, and compares every stored message as a bit
pattern (np.uint64, ==).  The restatement follows the kernel step by step: groups of four positions up to the wave's walk bound,
unused and dead positions reading the wave's far slot (64.0), `x <= 0` as the sign, strict `<` for the first-minimum position, the
butterfly merge of 2 or 4 partial walks (thread `sub` walks positions sub, sub + grp, ...), the re-read of the first-minimum
position's sign, the `live == 1` override, p = min * alpha, sign | magnitude stores in walk order, then the second minimum to the
first-minimum position, then the far slot re-armed.  No row is skipped: ROWS_MIN rows at least, counted."""
import numpy as np

FAR = -1          # slot number of the wave's far slot
CLIP = 50.0
ROWS_MIN = 10000


def walk(vals, slots, clip_each):
    """one thread's read phase over its positions (a multiple of four): min1, min2, first-minimum slot, sign bits"""
    min1 = min2 = 1e308
    arg = FAR
    neg = []
    for x, sl in zip(vals, slots):
        ax = min(abs(x), CLIP) if clip_each else abs(x)
        if ax < min1:
            arg = sl
        min2 = min(min2, max(min1, ax))
        min1 = min(min1, ax)
        neg.append(x <= 0)
    return [min1, min2, arg, sum(neg), neg]


def check_pass(msg, slots, synd, alpha, grp, wq, clip_each):
    """msg: {slot: value} of the live positions; slots: the check's positions in walk order (FAR for a dead one); grp threads share
    the check; wq: the wave's walk bound in positions per thread.  Returns the messages after the pass."""
    mem = dict(msg)
    mem[FAR] = 64.0
    live = sum(sl != FAR for sl in slots)
    walked = max(4, (wq + 3) & ~3)
    lanes = []
    for sub in range(grp):
        mine = slots[sub::grp]
        assert len(mine) <= walked
        mine = mine + [FAR] * (walked - len(mine))
        lanes.append((mine, walk([mem[sl] for sl in mine], mine, clip_each)))
    st = [list(w[:4]) for _, w in lanes]
    st[0][3] += synd                     # npar of sub 0 starts from the check's value
    x = 1
    while x < grp:                       # butterfly inside the quad: every lane ends with the merged result
        new = []
        for a in range(grp):
            m1, m2, arg, npar = st[a]
            o1, o2, oa, op = st[a ^ x]
            new.append([min(m1, o1), min(max(m1, o1), min(m2, o2)), oa if o1 < m1 else arg, npar + op])
        st = new
        x *= 2
    out = []
    for (mine, w), (m1, m2, arg, npar) in zip(lanes, st):
        if not clip_each:
            m1, m2 = min(m1, CLIP), min(m2, CLIP)
        argneg = mem[arg] <= 0           # re-read before the slots are overwritten
        if live == 1:
            m1 = m2 = 1e308
        out.append((mine, w[4], npar & 1, arg, argneg, m1 * alpha, m2 * alpha))
    for mine, neg, flip, arg, argneg, p1, p2 in out:       # the lanes run in lockstep: every group store ...
        for sl, ng in zip(mine, neg):
            mem[sl] = -p1 if (ng ^ flip) else p1
    for mine, neg, flip, arg, argneg, p1, p2 in out:       # ... then the second minimum
        mem[arg] = -p2 if (argneg ^ flip) else p2
    mem[FAR] = 64.0
    del mem[FAR]
    return mem


def bits(mem):
    return np.array([mem[k] for k in sorted(mem)], np.float64).view(np.uint64)


def both_ways(vals, dead_at=(), synd=0, alpha=0.9, grp=1, slack=0):
    """runs one row both ways and asserts equal bit patterns; vals: the live values in walk order, dead_at: positions (in the row with
    its dead positions) that are dead; returns the number of rows run (1)"""
    slots, it = [], iter(range(len(vals)))
    total = len(vals) + len(dead_at)
    for k in range(total):
        slots.append(FAR if k in dead_at else next(it))
    msg = {i: float(v) for i, v in enumerate(vals)}
    wq = (total + grp - 1) // grp + slack
    a = check_pass(msg, slots, synd, alpha, grp, wq, True)
    b = check_pass(msg, slots, synd, alpha, grp, wq, False)
    assert sorted(a) == sorted(b) == sorted(msg)
    assert np.array_equal(bits(a), bits(b)), (vals, dead_at, synd, alpha, grp, a, b)
    return 1


def reference_row(vals, synd, alpha):
    """the reference's statement of a row without dead positions: clip, then the minimum over the other edges"""
    x = np.clip(np.asarray(vals, np.float64), -50.0, 50.0)
    a, neg = np.abs(x), x <= 0
    par = (synd + int(neg.sum())) & 1
    out = []
    for j in range(len(x)):
        others = np.delete(a, j)
        mag = (others.min() if others.size else 1e308) * alpha
        out.append(-mag if (par ^ int(neg[j])) else mag)
    return np.array(out, np.float64).view(np.uint64)


POOLS = {
    "around 50": [49.0, 49.999999999999993, 50.0, 50.000000000000007, 51.0, 57.6, 3.5, 0.25],
    "around 64": [63.0, 63.999999999999993, 64.0, 64.000000000000014, 65.0, 69.1, 57.6, 12.0],
    "all above": [50.0, 50.000000000000007, 57.6, 63.9, 64.0, 64.5, 69.1, 1e3, 1e300],
    "zeros": [0.0, -0.0, 1.5, -1.5, 57.6, -69.1, 50.0, -50.0],
}


def random_row(rng, w, kind):
    if kind == "uniform":
        v = rng.uniform(-80.0, 80.0, size=w)
    elif kind == "one below":                       # exactly one value < 50
        v = rng.choice(POOLS["all above"], size=w) * rng.choice([-1.0, 1.0], size=w)
        v[rng.integers(w)] = rng.choice([0.0, -0.0, 1e-300, 7.25, -49.999999999999993])
    elif kind == "tie below":                       # the minimum twice or more, below the clip
        v = rng.uniform(-80.0, 80.0, size=w)
        t = rng.uniform(0.0, 49.0)
        for k in rng.choice(w, size=min(w, int(rng.integers(2, 4))), replace=False):
            v[k] = t * rng.choice([-1.0, 1.0])
        v = np.where(np.abs(v) < t, v + np.sign(v) * 50.0, v)
    elif kind == "tie at clip":                     # clipped minima tie at 50: different positions may be named first
        v = rng.choice(POOLS["all above"], size=w) * rng.choice([-1.0, 1.0], size=w)
    else:
        v = rng.choice(POOLS[kind], size=w) * rng.choice([-1.0, 1.0], size=w)
    return v.tolist()


def test_clip_once_stores_the_same_bits():
    rng = np.random.default_rng(15)
    kinds = ["uniform", "one below", "tie below", "tie at clip"] + list(POOLS)
    rows = 0
    per_kind = dict.fromkeys(kinds, 0)
    for r in range(ROWS_MIN + 800):
        kind = kinds[r % len(kinds)]
        w = int(rng.integers(2, 37))                # weight 2 .. 36
        vals = random_row(rng, w, kind)
        grp = (1, 2, 4)[r % 3] if w >= 4 else 1     # the row split over 2 and 4 partial walks and merged
        ndead = int(rng.integers(0, 5)) if r % 2 else 0
        dead_at = tuple(sorted(rng.choice(w + ndead, size=ndead, replace=False).tolist())) if ndead else ()
        if (w + ndead + grp - 1) // grp > 36:
            dead_at = ()
        rows += both_ways(vals, dead_at, synd=r & 1, alpha=(0.9, 1.0, 0.625)[r % 3], grp=grp, slack=int(rng.integers(0, 6)))
        per_kind[kind] += 1
    assert rows >= ROWS_MIN and min(per_kind.values()) >= 1000, (rows, per_kind)


def test_one_live_edge_and_dead_positions():
    rows = 0
    for x in (0.0, -0.0, 3.0, -3.0, 49.0, 50.0, 57.6, -57.6, 64.0, 69.1, -69.1):
        for ndead in (0, 1, 3, 7):
            for first in (False, True):             # the far slot may come first
                dead_at = tuple(range(ndead)) if first else tuple(range(1, 1 + ndead))
                for synd in (0, 1):
                    rows += both_ways([x], dead_at, synd=synd, slack=ndead % 3)
    # a partial walk that sees only dead positions and values >= 50 beside one that sees the small value
    for grp in (2, 4):
        for small_at in range(8):
            vals = [57.6, -69.1, 64.0, 50.0, 63.9, -57.6, 69.1, 51.0]
            vals[small_at] = -2.5
            rows += both_ways(vals, dead_at=(3, 9), synd=1, grp=grp)
            rows += both_ways(vals, synd=0, grp=grp, slack=2)
    assert rows == 11 * 4 * 2 * 2 + 2 * 8 * 2


def test_restatement_against_the_reference_rule():
    """the per-position form of this file is the reference's clip-then-minimum rule (rows without dead positions)"""
    rng = np.random.default_rng(16)
    for r in range(400):
        w = int(rng.integers(2, 37))
        vals = random_row(rng, w, ["uniform", "tie at clip", "zeros", "around 50"][r % 4])
        for clip_each in (True, False):
            got = check_pass(dict(enumerate(vals)), list(range(w)), r & 1, 0.9, (1, 2, 4)[r % 3] if w >= 4 else 1, (w + 3) // 1, clip_each)
            assert np.array_equal(bits(got), reference_row(vals, r & 1, 0.9)), (vals, clip_each)
