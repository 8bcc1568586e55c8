"""The column step of csrc/site_align.hip restated in Python with simulated threads, checked against the restatement of
test_site_align_cpu.py (no GPU).  What this covers is the decomposition the kernels rest on, not the kernels: a thread owns a block
of rows; a first walk leaves the vertical-gap value the block hands down (by extension, by opening in its last row); an exclusive
max-scan (passes (i), (ii)) or an in-order fold that also tells extension from opening (pass (iii)) gives the value that enters the
block; a second walk is the plain recurrence.  Also the echo window of pass (i), the early exit of pass (ii), the direction bytes and
the traceback.  Thread counts 4, 7 and 256 give blocks of many rows, ragged last blocks and blocks of one row."""
import numpy as np

import test_site_align_cpu as R

T = 256; NEG = -30000; NEG32 = -(1 << 28)
def score(qc, tc): return 5 if (qc == tc and tc < 4) else -4
def st(x): return min(max(x, NEG), 32767)

def sa_pass(MODE, q, tc, t0, q0, Rr, C, value, c_lo, nthreads=T):
    DIR = -1 if MODE == 1 else 1
    rpt = (Rr + nthreads - 1) // nthreads
    first = [min(Rr, t * rpt) for t in range(nthreads)]
    last = [min(Rr, first[t] + rpt) for t in range(nthreads)]
    init = 0 if MODE == 0 else NEG
    h = [[init] * Rr, [init] * Rr]; e = [init] * Rr
    key = 0; att = 0; dirs = {}; lastval = NEG
    for c in range(C):
        cur, nxt = h[c & 1], h[(c & 1) ^ 1]
        tcode = tc[t0 + DIR * c]
        top = 0 if MODE == 0 else (0 if c == 0 else NEG)
        oa = [NEG32] * nthreads; ob = [NEG32] * nthreads
        for t in range(nthreads):
            if first[t] < last[t]:
                hd = top if first[t] == 0 else cur[first[t] - 1]
                f = NEG32; hn = 0
                for r in range(first[t], last[t]):
                    hc = cur[r]; ee = max(e[r] - 4, hc - 16)
                    if r > first[t]: f = max(f - 4, hn - 16)
                    hh = max(hd + score(q[q0 + DIR * r], tcode), ee, f)
                    if MODE == 0: hh = max(hh, 0)
                    hd = hc; hn = hh
                oa[t] = f - 4; ob[t] = hn - 16
        fin = [NEG32] * nthreads; fin_ext = [0] * nthreads
        if MODE == 2:
            nact = (Rr + rpt - 1) // rpt
            for t in range(nthreads):
                fi = NEG32; fe = 0
                for k in range(nact):
                    if k >= t: break
                    ext = max(fi - 4 * rpt, oa[k]); opn = ob[k]
                    fi = max(ext, opn); fe = 1 if ext >= opn else 0
                fin[t], fin_ext[t] = fi, fe
        else:
            b = [max(oa[t], ob[t]) + 4 * rpt * t for t in range(nthreads)]
            ex = NEG32
            for t in range(nthreads):
                fin[t] = NEG32 if t == 0 else ex - 4 * rpt * (t - 1)
                ex = max(ex, b[t])
        newh = {}; newe = {}
        hit_rows = []
        for t in range(nthreads):
            fi = max(fin[t], NEG32)
            if first[t] < last[t]:
                hd = top if first[t] == 0 else cur[first[t] - 1]
                f = fi; hn = 0
                for r in range(first[t], last[t]):
                    hc = cur[r]; eo = e[r]; ee = max(eo - 4, hc - 16)
                    fext = fin_ext[t]
                    if r > first[t]:
                        fext = 1 if f - 4 >= hn - 16 else 0
                        f = max(f - 4, hn - 16)
                    dg = hd + score(q[q0 + DIR * r], tcode)
                    hh = max(dg, ee, f)
                    if MODE == 0:
                        hh = max(hh, 0)
                        if c >= c_lo and hh == value:
                            key = max(key, ((c - c_lo + 1) << 20) | (0xfffff - r))
                            if c == C - 1 or r == Rr - 1: att = 1
                    if MODE == 1 and dg == value: hit_rows.append(r)
                    if MODE == 2:
                        src = 0 if hh == dg else (1 if hh == ee else 2)
                        dirs[(c, r)] = src | (4 if ee == eo - 4 else 0) | (8 if fext else 0)
                        if c == C - 1 and r == Rr - 1: lastval = hh
                    newh[r] = st(hh); newe[r] = st(ee)
                    hd = hc; hn = hh
        for r, v in newh.items(): nxt[r] = v
        for r, v in newe.items(): e[r] = v
        if MODE == 1 and hit_rows:
            return c, min(hit_rows)
    if MODE == 0: return key, att
    if MODE == 1: return -1, -1
    return lastval, dirs

def traceback(dirs, Rr, C):
    r, c, state, run, run_op, out = Rr - 1, C - 1, 0, 0, 0, []
    for step in range(2 * (Rr + C) + 4):
        if r < 0 or c < 0: break
        d = dirs[(c, r)]
        if state == 0:
            src = d & 3
            if src == 1: state = 1; continue
            if src == 2: state = 2; continue
            op = 0; r -= 1; c -= 1
        elif state == 1:
            op = 2
            if not d & 4: state = 0
            c -= 1
        else:
            op = 1
            if not d & 8: state = 0
            r -= 1
        if run > 0 and op != run_op:
            out.append((run, run_op)); run = 0
        run_op = op; run += 1
    assert r == -1 and c == -1 and state == 0, (r, c, state)
    out.append((run, run_op))
    out.reverse()
    return "".join(f"{n}{'MID'[o]}" for n, o in out)

def kernel_hit(rna, target, jp, value, nthreads):
    q = [int(R._CODE[x]) for x in rna]; tc = [int(R._CODE[x]) for x in target]
    m = len(q); npad = 16 * ((m + 15) // 16) - m
    c_lo = max(0, jp - npad)
    key, att = sa_pass(0, q, tc, 0, 0, m, jp + 1, value, c_lo, nthreads)
    assert key and att, (key, att)
    j1 = c_lo + (key >> 20) - 1; i1 = 0xfffff - (key & 0xfffff)
    c, r = sa_pass(1, q, tc, j1, i1, i1 + 1, j1 + 1, value, 0, nthreads)
    assert c >= 0
    j0, i0 = j1 - c, i1 - r
    lastval, dirs = sa_pass(2, q, tc, j0, i0, i1 - i0 + 1, j1 - j0 + 1, value, 0, nthreads)
    assert lastval == value
    return i0, i1, j0, j1, traceback(dirs, i1 - i0 + 1, j1 - j0 + 1)


def test_thread_blocked_column_step_equals_the_restatement():
    rng = np.random.default_rng(5)
    n_ok, seen = 0, set()
    for trial in range(30):
        m = int(rng.integers(34, 90))
        n = int(rng.integers(60, 160))
        qy, t = R._planted(rng, m, n, trial % 3, at_end=trial % 4 == 3)
        if trial % 5 == 0:                     # low complexity: many ties and gaps
            qy = bytes(rng.choice(list(b"GT"), size=m).astype(np.uint8).tobytes())
            t = bytes(rng.choice(list(b"GTN"), size=n).astype(np.uint8).tobytes())
        H = R.unit_matrix(qy, t)
        cm = H.max(axis=0)
        value = int(cm.max())
        if value < 5:
            continue
        for jp in sorted({int(np.argmax(cm)), int(np.flatnonzero(cm == value)[-1])}):
            want = R.align_in_unit(qy, t, H, jp, value)
            for nth in (4, 7, 256):
                assert kernel_hit(qy, t, jp, value, nth) == want, (trial, jp, nth, want)
                n_ok += 1
            seen |= set(want[4]) & set("ID")
    assert n_ok >= 90 and seen == {"I", "D"}
