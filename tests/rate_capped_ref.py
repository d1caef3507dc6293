"""The NumPy restatement of capped rate control (include/vrvq.h "Capped rate control"), built on
the restatement of tests/test_rate.py: the cap of a packet is solve_level on that packet alone,
and the group's level is the same bisection over the float32 bit patterns with every packet at
min(level, cap). Totals are Python ints and levels np.float32, so everything compared with it is
compared by equality. Shared by tests/test_rate_capped.py and tests/test_gpu_rate_capped.py, with
the inputs the issue fixes for both."""
import numpy as np

from test_rate import solve_level, total_bits

LO, HI = 0.125, 6.0


def bits_table(nq, uniform):
    return [10] * nq if uniform else [10 - (i // 2) % 3 for i in range(nq)]  # test_gpu_rate.py's


def packets_of(T, P):
    return (T - 1) // P + 1


def packet_frames_of(T, P):
    """Frames of every packet of a row: P, and what is left for the last one."""
    return [min(P, T - p * P) for p in range(packets_of(T, P))]


def packet_caps(imp, P, nq, bits, packet_budget, lo, hi):
    """(cap (B, NP) float32, infeasible (B, NP) bool): solve_level of every packet on its own."""
    B, T = imp.shape
    NP = packets_of(T, P)
    cap = np.zeros((B, NP), np.float32)
    bad = np.zeros((B, NP), bool)
    for b in range(B):
        for p in range(NP):
            lv, _, st = solve_level(imp[b, p * P:(p + 1) * P], nq, bits, packet_budget[p], lo, hi)
            cap[b, p], bad[b, p] = lv, st == 1
    return cap, bad


def packet_totals(imp, P, levels, nq, bits):
    """Bits of every packet at its own level, (B, NP) int64."""
    B, NP = levels.shape
    return np.array([[total_bits(imp[b, p * P:(p + 1) * P], levels[b, p], nq, bits)
                      for p in range(NP)] for b in range(B)], np.int64).reshape(B, NP)


def capped_total(imp, P, cap, level, nq, bits):
    """Bits of the rows of imp with every packet at min(level, its cap), a Python int."""
    return int(packet_totals(imp, P, np.minimum(np.float32(level), cap), nq, bits).sum())


def solve_group_capped(imp, P, cap, nq, bits, budget, lo, hi):
    """(lambda, total, status) of one group of rows: solve_level with capped_total for
    total_bits."""
    lo, hi = np.float32(lo), np.float32(hi)
    t_lo = capped_total(imp, P, cap, lo, nq, bits)
    if t_lo > budget:
        return lo, t_lo, 1
    t_hi = capped_total(imp, P, cap, hi, nq, bits)
    if t_hi <= budget:
        return hi, t_hi, 2
    a, b, tot = int(lo.view(np.uint32)), int(hi.view(np.uint32)), t_lo
    while b - a > 1:
        m = a + (b - a) // 2
        t = capped_total(imp, P, cap, np.uint32(m).view(np.float32), nq, bits)
        if t <= budget:
            a, tot = m, t
        else:
            b = m
    return np.uint32(a).view(np.float32), tot, 0


def solve_capped(imp, P, nq, bits, group_off, budgets, packet_budget, lo=LO, hi=HI):
    """All six outputs of vrvq_rate_solve_capped for groups that share no rows: level (G,)
    float32, total (G,) int64, status (G,) int32, packet_level (B, NP) float32, packet_total
    (B, NP) int64, packet_status (B, NP) int32. A row of no valid group keeps its caps, the totals
    at them and state 1 (infeasible) or 2."""
    imp = np.asarray(imp, np.float32)
    B, T = imp.shape
    G = len(group_off) - 1
    cap, bad = packet_caps(imp, P, nq, bits, packet_budget, lo, hi)
    level = np.zeros(G, np.float32)
    total = np.zeros(G, np.int64)
    status = np.zeros(G, np.int32)
    p_level = cap.copy()
    p_status = np.where(bad, 1, 2).astype(np.int32)
    for g in range(G):
        r0, r1 = group_off[g], group_off[g + 1]
        if r0 < 0 or r1 < r0 or r1 > B:
            level[g], total[g], status[g] = lo, 0, -1
        elif r0 == r1:
            level[g], total[g], status[g] = hi, 0, 2
        else:
            lam, tot, st = solve_group_capped(imp[r0:r1], P, cap[r0:r1], nq, bits, budgets[g],
                                              lo, hi)
            level[g], total[g], status[g] = lam, tot, st
            p_level[r0:r1] = np.minimum(lam, cap[r0:r1])
            p_status[r0:r1] = np.where(bad[r0:r1], 1, np.where(cap[r0:r1] < lam, 2, 0))
    return level, total, status, p_level, packet_totals(imp, P, p_level, nq, bits), p_status


# ------------------------------------------------------------------ the inputs of the issue
# (B, T, P, nq): the smallest shape; a tail packet of 2; a tail of 1 and non-uniform bits; P > T;
# P = T; 4096 / 4097 elements, the bound between a group held in registers and one read again; the
# re-read path with packets that straddle its 4096-element tiles (pooled); 5000 frames in a row.
# Every shape is solved per clip and pooled.
SHAPES = [(1, 1, 1, 8), (3, 50, 16, 9), (2, 257, 64, 32), (2, 40, 64, 9), (4, 87, 87, 9),
          (3, 87, 20, 28), (1, 4096, 256, 8), (1, 4097, 256, 8), (5, 1000, 87, 28),
          (1, 5000, 256, 8)]


def checkerboard(B, T, P):
    """The gain of every frame, (B, T): 1 or 0.25 in a checkerboard over (row, packet), so that
    dense packets (which a cap binds) alternate with sparse ones (which it does not)."""
    NP = packets_of(T, P)
    gain = np.array([[1.0 if (b + p) % 2 == 0 else 0.25 for p in range(NP)] for b in range(B)],
                    np.float32)
    return np.repeat(gain, P, axis=1)[:, :T]


def make_imp(B, T, P):
    """u * gain: u uniform in (0, 1), the gain of checkerboard()."""
    u = np.random.default_rng(7 * B + T).random((B, T), dtype=np.float32)
    u[u == 0] = 0.5
    return u * checkerboard(B, T, P)


def make_case(B, T, P, nq, pooled):
    """imp, bits, group_off, budgets, packet_budget of one shape: the group budget 6/10 of the way
    from the total at LO to the total at HI, a packet's 0.7 of all its codes."""
    imp = make_imp(B, T, P)
    bits = bits_table(nq, nq != 32)                 # (2, 257, 64, 32): non-uniform bits
    off = [0, B] if pooled else list(range(B + 1))
    budgets = []
    for g in range(len(off) - 1):
        rows = imp[off[g]:off[g + 1]]
        t_lo, t_hi = total_bits(rows, LO, nq, bits), total_bits(rows, HI, nq, bits)
        budgets.append(t_lo + (t_hi - t_lo) * 6 // 10)
    packet_budget = [int(0.7 * sum(bits) * n) for n in packet_frames_of(T, P)]
    return imp, bits, off, budgets, packet_budget


_cases = {}


def case(shape, pooled):
    """(inputs, restatement outputs) of one of SHAPES, computed once and shared."""
    if (shape, pooled) not in _cases:
        inputs = make_case(*shape, pooled)
        imp, bits, off, budgets, packet_budget = inputs
        _cases[shape, pooled] = (inputs, solve_capped(imp, shape[2], shape[3], bits, off, budgets,
                                                      packet_budget))
    return _cases[shape, pooled]
