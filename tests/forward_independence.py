"""A board's (policy, value) is a function of that board and of the kernel that ran it: the checks, as plain functions of a
callable (tests/test_forward_independence_host.py runs them on a stand-in on the CPU, tests/test_gpu_forward_independence.py on
every kernel name of the network forward).

Every network kernel evaluates many boards at once: 16 or 32 to an MFMA group, or one board per workgroup. The search tests
move games between rows (refills, carry-over, over-subscription, the rolling search) and replay evaluation logs, and all of them
lean on the result of a board not depending on the row it sits in, on the boards around it or on how ragged the last group is.
The precision tests hold every row to float64 within about 1e-6 in a logit; a stale low fp16 half of a neighbour's row, a
summation order that depends on the lane or a tail group that pads differently stays far inside that, and "two forwards of
the same batch are equal" cannot see a defect that is a deterministic function of the row. What is asked here needs no
reference and no tolerance: equality of bits.

`fwd(x) -> (p, v)`: x [n, C, B, B] float32 numpy, p [n, A] and v [n] float32 numpy. Bits (`view(np.uint32)`) are compared,
never values. The five checks, at one batch size n (one kernel):

  twins        a batch in which a board sits at every probe row (0, 15, 16, the middle, the first and last row of the last
               group, n - 1) -- once a lively board (float planes), once the full board -- among net_reference.batch_indices'
               draw: all rows that hold the same pool board have equal bits;
  constant     every row holds the lively board: all rows equal, and equal to that board's rows of the twins batch;
  permutation  fwd(x[perm]) == fwd(x)[perm] for a reversal with a shift (a rotation at 36 .. 56 boards), which sends at least nine
               rows in ten to another group AND another lane;
  neighbours   every row that is not a probe row replaced by a board of another pool: the probe rows keep their bits;
  tail         the last row dropped (only where the library names the same kernel for n - 1): rows 0 .. n-2 keep their bits.

A failure raises Mismatch (an AssertionError) whose message names the check, the kernel, the two rows with index, row // 16 and
row % 16, the pool board and the first differing cell."""
import numpy as np

import net_reference as R

CHECKS = ("twins", "constant", "permutation", "neighbours", "tail")
COVERAGE = 0.9          # share of the rows a permutation must send to another group and another lane, from 33 boards on


class Mismatch(AssertionError):
    def __init__(self, check, message):
        super().__init__(message)
        self.check = check


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def probe_rows(n):
    """0, 15, 16, n - 1, the first and last row of the last 16-board group and one row in the middle: what fits into n."""
    last = (n - 1) // 16 * 16
    return sorted({r for r in (0, 15, 16, n // 2, last, n - 1) if 0 <= r < n})


def lively_board(B, C=5):
    """Pool index of the float-plane board the twins and constant batches repeat ("float planes 1": values that are neither
    0/1 nor fp16 numbers on 5 % of the cells, so both fp16 halves of conv1's input are in use)."""
    names = R.structured_boards(B, C)[1]
    return names.index("float planes 1")


def full_board(B, C=5):
    return R.structured_boards(B, C)[1].index("full")


def twins_indices(n, B, C, board):
    """net_reference.batch_indices(n, B, C) with pool board `board` written over the probe rows."""
    m = np.array(R.batch_indices(n, B, C))
    m[probe_rows(n)] = board
    return m


def coverage(perm):
    """Share of the rows of x[perm] that hold a row of x from another 16-board group AND another lane of a group."""
    to = np.arange(len(perm))
    return float(((perm // 16 != to // 16) & (perm % 16 != to % 16)).mean())


def permutation(n):
    """(np.arange(n)[::-1] + shift) % n with the first shift of 7, 8, 9, ... that moves at least 90 % of the rows to another
    group and another lane. A reversal leaves the rows around its two centres in their group, and for an even n + shift one row
    in eight in its lane: 7 itself misses the condition at most batch sizes below 200, and from 36 to about 56 boards (three
    or four groups, up to 32 rows around the centres) every shift does. There the permutation is the first rotation
    (np.arange(n) + shift) % n, shift = 17, 18, ..., that meets it. Fewer than 33 boards have no such permutation: shift 7."""
    rev = np.arange(n)[::-1]
    if n < 33:
        return (rev + 7) % n
    for shift in range(7, 7 + n):
        perm = (rev + shift) % n
        if coverage(perm) >= COVERAGE:
            return perm
    for shift in range(17, n):
        perm = (np.arange(n) + shift) % n
        if coverage(perm) >= COVERAGE:
            return perm
    raise AssertionError("no shifted reversal or rotation of %d rows moves %d %% of them to another group and lane" % (n, 100 * COVERAGE))


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def bits(out):
    """(p, v) float32 -> uint32 [n, A + 1]: a row's policy bits, then its value bits."""
    p, v = out
    p, v = np.ascontiguousarray(p), np.ascontiguousarray(v)
    assert p.dtype == np.float32 and v.dtype == np.float32 and p.ndim == 2 and v.shape == (p.shape[0],), (p.dtype, v.dtype, p.shape, v.shape)
    return np.concatenate([p.view(np.uint32), v.view(np.uint32)[:, None]], axis=1)


def _row(r):
    return "row %d (group %d, lane %d)" % (r, r // 16, r % 16)


def same_rows(check, kernel, a, rows_a, b, rows_b, boards, what_a="", what_b=""):
    """bits a[rows_a[k]] == bits b[rows_b[k]] for every k; boards[k] names the pool board the two rows hold."""
    rows_a, rows_b = np.asarray(rows_a, np.int64), np.asarray(rows_b, np.int64)
    if rows_a.size == 0:
        return
    ba, bb = a[rows_a], b[rows_b]
    bad = np.flatnonzero((ba != bb).any(axis=1))
    if bad.size == 0:
        return
    k = int(bad[0])
    cell = int(np.flatnonzero(ba[k] != bb[k])[0])
    A = a.shape[1] - 1
    where = "value" if cell == A else "policy cell %d" % cell
    x, y = ba[k, cell:cell + 1].view(np.float32)[0], bb[k, cell:cell + 1].view(np.float32)[0]
    raise Mismatch(check, "%s, %s: %s%s and %s%s hold pool board %s and differ, first at %s: %r (0x%08x) against %r (0x%08x); "
                          "%d of %d compared row pairs differ"
                   % (check, kernel, _row(int(rows_a[k])), what_a, _row(int(rows_b[k])), what_b, boards[k], where, x, int(ba[k, cell]),
                      y, int(bb[k, cell]), bad.size, rows_a.size))


# ------------------------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------------------------
class Checker:
    """The five checks of one (fwd, kernel, batch size). pool / other: the boards [N, C, B, B] the batches are drawn from and
    the boards the neighbours check puts around the probe rows; lively / full: indices into pool. Every forward's output is
    kept, so a check that shares a batch with another does not run it again."""

    def __init__(self, fwd, kernel, n, B, C, pool=None, other=None, lively=None, full=None):
        self.fwd, self.kernel, self.n, self.B, self.C = fwd, kernel, n, B, C
        self.pool = R.pool(B, C) if pool is None else pool
        self.other = R.pool(B, C, seed=1) if other is None else other
        self.lively = lively_board(B, C) if lively is None else lively
        self.full = full_board(B, C) if full is None else full
        self.probes = probe_rows(n)
        self.ran = []
        self._twins = {}

    def _run(self, x):
        out = bits(self.fwd(np.ascontiguousarray(x, np.float32)))
        assert out.shape[0] == len(x), (out.shape, len(x))
        return out

    def _twins_batch(self, board):
        if board not in self._twins:
            m = twins_indices(self.n, self.B, self.C, board)
            self._twins[board] = (m, self._run(self.pool[m]))
        return self._twins[board]

    def twins(self):
        for board in (self.lively, self.full):
            m, out = self._twins_batch(board)
            order = np.argsort(m, kind="stable")
            first = {}
            ra, rb = [], []
            for r in order:                                   # every row against the first row that holds its board
                if m[r] in first:
                    ra.append(first[m[r]])
                    rb.append(r)
                else:
                    first[m[r]] = r
            same_rows("twins", self.kernel, out, ra, out, rb, [int(m[r]) for r in rb])
        self.ran.append("twins")

    def constant(self):
        out = self._run(self.pool[np.full(self.n, self.lively)])
        rows = np.arange(1, self.n)
        same_rows("constant", self.kernel, out, np.zeros_like(rows), out, rows, [self.lively] * len(rows))
        m, tw = self._twins_batch(self.lively)
        rows = np.flatnonzero(m == self.lively)
        same_rows("constant", self.kernel, out, rows, tw, rows, [self.lively] * len(rows), " of the constant batch", " of the twins batch")
        self.ran.append("constant")

    def permutation(self):
        m, out = self._twins_batch(self.lively)
        perm = permutation(self.n)
        moved = self._run(self.pool[m[perm]])
        same_rows("permutation", self.kernel, moved, np.arange(self.n), out, perm, [int(b) for b in m[perm]], " of the permuted batch",
                  " of the batch")
        self.ran.append("permutation")

    def neighbours(self):
        m, out = self._twins_batch(self.lively)
        x = np.array(self.pool[m])
        rest = np.setdiff1d(np.arange(self.n), self.probes)
        rs = np.random.RandomState(self.n + 131 * self.B)
        x[rest] = self.other[rs.randint(0, len(self.other), size=len(rest))]
        new = self._run(x)
        same_rows("neighbours", self.kernel, new, self.probes, out, self.probes, [self.lively] * len(self.probes), " among other boards", "")
        self.ran.append("neighbours")

    def tail(self):
        if self.n < 2:
            return
        m, out = self._twins_batch(self.lively)
        short = self._run(self.pool[m[:-1]])
        rows = np.arange(self.n - 1)
        same_rows("tail", self.kernel, short, rows, out, rows, [int(b) for b in m[:-1]], " of %d boards" % (self.n - 1), " of %d boards" % self.n)
        self.ran.append("tail")

    def run(self, tail=True):
        """All checks (tail: whether n - 1 boards run the same kernel); the first failure raises."""
        self.twins()
        self.constant()
        self.permutation()
        self.neighbours()
        if tail:
            self.tail()
        return list(self.ran)

    def failures(self, tail=True):
        """{check: message} of the checks that fail, every check run."""
        out = {}
        for name in CHECKS:
            if name == "tail" and not tail:
                continue
            try:
                getattr(self, name)()
            except Mismatch as e:
                out[e.check] = str(e)
        return out
