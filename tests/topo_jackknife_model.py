"""The block jackknife of `Colate --mode count_topo --jackknife` (csrc/count_topo.h) restated in plain Python: Python's float is the
IEEE double of the C++, float(int) rounds as (double)(long long) does, and every operation below is one rounded operation in the
order the header states.  Independent of the C++: no numpy arithmetic, no library call."""
import math

NAN = float("nan")


def cell_blocks(counts, cell):
    """[(a_j, b_j)] of one cell over the blocks: epoch `cell`, or the sum over the epochs where cell == E; counts [nb][E][3]"""
    E = len(counts[0])
    out = []
    for block in counts:
        es = range(E) if cell == E else (cell,)
        out.append((sum(int(block[e][0]) for e in es), sum(int(block[e][1]) for e in es)))
    return out


def jackknife_cell(blocks):
    """(D, D_jack, se, Z, g) of one cell from [(a_j, b_j)]"""
    used = [(a, b) for a, b in blocks if a + b > 0]
    g = len(used)
    A, M = sum(a for a, _ in used), sum(b for _, b in used)
    n = A + M
    if n == 0:
        return NAN, NAN, NAN, NAN, g
    D = float(A - M) / float(n)
    if g < 2:
        return D, NAN, NAN, NAN, g
    theta = [float((A - a) - (M - b)) / float(n - (a + b)) for a, b in used]
    h = [float(n) / float(a + b) for a, b in used]
    s = 0.0
    for (a, b), th in zip(used, theta):
        s += (float(n - (a + b)) / float(n)) * th
    D_jack = float(g) * D - s
    v = 0.0
    for hj, th in zip(h, theta):
        tau = hj * D - (hj - 1.0) * th
        d = tau - D_jack
        v += (d * d) / (hj - 1.0)
    se = math.sqrt(v / float(g))
    Z = D_jack / se if se > 0 else NAN
    return D, D_jack, se, Z, g


def jackknife(counts):
    """(stats [E + 1][4], used [E + 1]) of one triple's counts [nb][E][3]"""
    E = len(counts[0])
    cells = [jackknife_cell(cell_blocks(counts, cell)) for cell in range(E + 1)]
    return [list(c[:4]) for c in cells], [c[4] for c in cells]


def number(x):
    return "NA" if math.isnan(x) else "%.6g" % x


def lines(names, printed_epochs, counts):
    """the lines of PREFIX.jackknife.txt of one triple: names "cond target reference", the epochs as PREFIX.profile.txt prints them"""
    E = len(counts[0])
    stats, used = jackknife(counts)
    out = []
    for cell in range(E + 1):
        blocks = cell_blocks(counts, cell)
        plus, minus = sum(a for a, _ in blocks), sum(b for _, b in blocks)
        out.append(" ".join([names, printed_epochs[cell] if cell < E else "all", str(plus), str(minus), str(used[cell])] + [number(x) for x in stats[cell]]))
    return out
