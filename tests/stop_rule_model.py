"""A plain Python restatement of the device's phase-2 policy between "candidates" and "rows" (csrc/k_phase2.hip, csrc/host_phase2.hip),
run on the oracle's walk (oracle.Result.walk): which ranks a round aligns (k_round_counts), how k_stop_round_w replays the sequential
rule over them -- 64 ranks per ballot step, or rank by rank when a candidate has tiles -- and what k_final_select* reports.

`dev` names ONE deviation from the code as written (DEVIATIONS); tests/test_stop_rule.py shows which designed case tells each of them
from the oracle.
"""
import math

DEVIATIONS = {
    "gt_for_ge": "unmch > mmiss in place of unmch >= mmiss",
    "floor_for_ceil": "a round sized by floor(mmiss) in place of ceil(mmiss)",
    "unmch_not_carried": "unmch restarts at 0 with every round",
    "mask_at_used_64": "nsel counted through (1 << used) - 1 at used == 64 too (the shift wraps: an empty mask)",
    "bv_per_rank": "bv counts a rank with passing tiles once, not its passing tiles",
    "vmax_plus_1": "the task list holds vmax + 1 ranks",
    "nout_without_v": "nout = nsel, without the cap of v",
}


def vmax_of(v):
    return max(100, max(v + 100, int(v * 1.1)))   # fsearch.py:3059


def _rank(walk, r):
    """(tasks, hits per tile or None, bits, cells or None) of rank r; a rank the walk does not list is one missing task"""
    if r < len(walk["ranks"]):
        k = walk["ranks"][r]
        return k["tasks"], k["hits"], k["bits"], k["cells"]
    return 1, None, None, None


def model_stop(walk, first, count, state, v, dev=None):
    """k_stop_round_w over ranks [first, first + count): state = [next, unmch, bv, nsel, done] is advanced, `sel` (position -> (rank,
    tile)) filled; -> (bit of the stop inside the round or None, whether the rule looked at a rank the walk knows no verdict of)"""
    mm = walk["mmiss"]
    r, unmch, bv, nsel = state[:4]
    sel = state[5]
    nt = state[6]
    done, stop_bit, blind = False, None, False

    def fires():
        miss = unmch > mm if dev == "gt_for_ge" else unmch >= mm
        return miss or float(bv) >= float(v) + mm

    ranks = [_rank(walk, first + k) for k in range(count)]
    if any(t[0] != 1 for t in ranks):
        # tiled candidates: the serial walk
        for k, (tasks, hits, _, _) in enumerate(ranks):
            if hits is None and tasks:
                blind, hits = True, [0] * tasks
            hit = False
            for t in range(tasks):
                if hits[t]:
                    sel[nsel] = (first + k, t)
                    nsel += 1
                    if dev != "bv_per_rank" or not hit:
                        bv += 1
                    hit = True
            unmch = 0 if hit else unmch + 1
            r += 1
            if fires():
                done, stop_bit = True, k
                break
    else:
        for c0 in range(0, count, 64):
            if done:
                break
            cnt = min(64, count - c0)
            hb = 0
            for i in range(cnt):
                hits = ranks[c0 + i][1]
                if hits is None:
                    blind, hits = True, [0]
                hb |= (1 if hits[0] else 0) << i
            used = cnt
            for i in range(cnt):
                if (hb >> i) & 1:
                    unmch, bv = 0, bv + 1
                else:
                    unmch += 1
                if fires():
                    done, used, stop_bit = True, i + 1, c0 + i
                    break
            for lane in range(used):
                if (hb >> lane) & 1:
                    sel[nsel + bin(hb & ((1 << lane) - 1)).count("1")] = (first + c0 + lane, 0)
            if used >= 64 and dev != "mask_at_used_64":
                nsel += bin(hb).count("1")
            else:
                nsel += bin(hb & ((1 << (used & 63)) - 1)).count("1")   # (a 64-bit shift by 64 is a shift by 0)
            r += used
    if r >= nt:
        done = True
    state[0:5] = [r, unmch, bv, nsel, 1 if done else 0]
    return stop_bit, blind


def model_query(walk, v, dev=None, qsort=None):
    """The whole chain for one query -> dict: state (next, unmch, bv, nsel, done), ntask, ntile, ranks / tasks aligned, cells (None when an
    aligned rank has none: walk without shadow), rounds [(first rank, ranks, unmch behind it)], stop (round, bit) or None, blind, and with
    `qsort` (the reference quicksort: keys -> permutation) the reported selection [(rank, tile)]"""
    mm = walk["mmiss"]
    nt = min(walk["ncand"], vmax_of(v) + (1 if dev == "vmax_plus_1" else 0))
    ntile = sum(_rank(walk, r)[0] for r in range(nt))
    cm = math.floor(mm) if dev == "floor_for_ceil" else math.ceil(mm)
    state = [0, 0, 0, 0, 0, {}, nt]
    minr, rounds, stop, blind = 8, [], None, False
    ranks_al = tasks_al = 0
    cells = 0
    while not state[4] and state[0] < nt:   # (a query without ranks never reaches k_stop_round_w: its state stays 0, done included)
        if dev == "unmch_not_carried":
            state[1] = 0
        need = max(cm - state[1] if cm > state[1] else 1, minr)   # k_round_counts
        count = min(nt - state[0], need)
        first = state[0]
        for r in range(first, first + count):
            tasks, _, _, cl = _rank(walk, r)
            tasks_al += tasks
            if cells is not None:
                cells = None if (cl is None and tasks) else cells + sum(cl or [])
        ranks_al += count
        bit, bl = model_stop(walk, first, count, state, v, dev)
        blind = blind or bl
        rounds.append((first, count, state[1]))
        if bit is not None:
            stop = (len(rounds), bit)
        minr = minr * 2 if minr < 256 else minr
    nsel = state[3]
    out = dict(state=tuple(state[:5]), ntask=nt, ntile=ntile, ranks=ranks_al, tasks=tasks_al, cells=cells, rounds=rounds, stop=stop, blind=blind)
    if qsort is not None:
        sel = [state[5].get(i) for i in range(nsel)]
        if any(s is None for s in sel):
            out["selection"] = None   # (a position never written: only a deviation gets here)
        else:
            keys = [-_rank(walk, r)[2][t] if _rank(walk, r)[2] else 0 for r, t in sel]
            order = qsort(keys)
            nout = nsel if dev == "nout_without_v" else min(nsel, max(v, 0))
            out["selection"] = [sel[i] for i in order[:nout]]
    return out


def model_rounds(walk, v):
    """the present round policy alone: ranks aligned, tasks aligned, and their cells (None without shadow)"""
    m = model_query(walk, v)
    return dict(ranks=m["ranks"], tasks=m["tasks"], cells=m["cells"])


def observable(m):
    """what a test can see of a model run: the read-out's fields, the work counters and the reported selection"""
    return (m["state"], m["ntask"], m["ntile"], m["tasks"], m["cells"], tuple(m["selection"]) if m.get("selection") is not None else None)
