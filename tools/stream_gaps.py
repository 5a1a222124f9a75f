"""Per-stream launch gaps of ONE replayed KD step out of a rocprofv3 --kernel-trace result (rocpd sqlite .db).

    python tools/stream_gaps.py <kd_results.db> <out.md> [period] [from_kernel_substring]

The step is chosen as tools/step_sequence.py chooses it (the middle one of the most frequent dispatch count; `period`
steps per unit with the grouped teacher pass).  A replayed hipGraph reports ONE stream id for all its nodes (the stream it
was launched on), whatever streams they were captured on, so the student's chain is told apart by name: it is every
kernel of the stream that carries the optimiser launch EXCEPT the weight gradients the sweep forks (`conv_wgrad*`,
`wgrad_group*`).  Every chain kernel is printed with `start - end of the previous chain kernel`, the hardware queue the
trace reports for it, and what started inside that gap: forked weight gradients, and kernels of other streams (the
teacher's segment).  The summary splits the gaps by whether a weight gradient started inside them.

`from_kernel_substring` limits the table (not the summary) to the part of the step behind the first kernel whose name
contains it, e.g. `loss_backward` for the reverse sweep.

Under the tracer a hipGraph's nodes may be replayed one at a time (tools/step_sequence.py): a gap in this table is a gap
of the TRACED schedule.  Whether the untraced step has it is what `bench.py --timeline` (device timestamps from inside
the graph) says.
"""
import sqlite3
import sys

from rocprof_summary import short


def load(db):
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("PRAGMA table_info(kernels)")]
    pick = lambda *names: next((n for n in names if n in cols), None)      # noqa: E731
    c_start, c_end = pick("start", "start_ns"), pick("end", "end_ns")
    c_stream, c_queue = pick("stream_id", "stream"), pick("queue_id", "queue")
    sel = "name, %s, %s, %s, %s" % (c_start, c_end, c_stream or "0", c_queue or "0")
    return list(c.execute("select %s from kernels order by %s" % (sel, c_start))), c_stream


def pick_step(rows, period):
    opt = [i for i, r in enumerate(rows) if "clip_adamw" in r[0]]
    if len(opt) < 3:
        raise SystemExit("need at least 3 optimizer launches in the trace, found %d" % len(opt))
    best = None
    for off in range(period):
        spans = [(opt[i - period] + 1, opt[i]) for i in range(period + off, len(opt), period)]
        by_len = {}
        for sp in spans:
            by_len.setdefault(sp[1] - sp[0] + 1, []).append(sp)
        if not by_len:
            continue
        n_mode, group = max(by_len.items(), key=lambda kv: len(kv[1]))
        if best is None or len(group) > len(best[1]):
            best = (n_mode, group)
    lo, hi = best[1][len(best[1]) // 2]
    return rows[lo:hi + 1], best[0], len(best[1])


def forked(name):
    return "conv_wgrad" in name or "wgrad_group" in name


def gaps(step):
    """[(index, name, start, dur, gap or None, [names of the kernels outside the chain that started inside the gap],
    queue)] of the chain = the optimiser's stream without the forked weight gradients."""
    main = next(r[3] for r in reversed(step) if "clip_adamw" in r[0])
    chain = lambda r: r[3] == main and not forked(r[0])      # noqa: E731
    out, prev_end = [], None
    for i, r in enumerate(step):
        if not chain(r):
            continue
        name, s, e, _, q = r
        between = []
        if prev_end is not None:
            between = [short(o[0]) for o in step if not chain(o) and prev_end <= o[1] < s]
        out.append((i, name, s, e - s, None if prev_end is None else s - prev_end, between, q))
        prev_end = max(e, prev_end or e)
    return main, out


def main():
    db, out = sys.argv[1], sys.argv[2]
    period = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    since = sys.argv[4] if len(sys.argv) > 4 else ""
    rows, c_stream = load(db)
    step, n_mode, n_like = pick_step(rows, period)
    main_q, table = gaps(step)
    t0 = step[0][1]
    streams = sorted({r[3] for r in step}, key=str)
    lines = ["# per-stream launch gaps of one replayed KD %s (rocprofv3 --kernel-trace)" %
             ("step" if period == 1 else "period of %d steps" % period), "",
             "source: `%s`; %d dispatches in the unit (%d like it in the trace); stream column: `%s`, values %s; the "
             "optimiser's stream: %s" % (db, n_mode, n_like, c_stream, streams, main_q), ""]
    with_fork = [t for t in table if t[4] is not None and any(forked(b) for b in t[5])]
    other = [t for t in table if t[4] is not None and t[5] and t not in with_fork]
    plain = [t for t in table if t[4] is not None and not t[5]]

    def stat(name, ts):
        g = sorted(t[4] / 1e3 for t in ts)
        if not g:
            return "| %s | 0 | | | | |" % name
        return "| %s | %d | %.1f | %.1f | %.1f | %.1f |" % (name, len(g), sum(g), g[len(g) // 2], g[0], g[-1])

    lines += ["| gaps of the chain | count | total us | median us | min us | max us |", "|---|---|---|---|---|---|",
              stat("a forked weight gradient started inside", with_fork),
              stat("only kernels of another stream started inside", other),
              stat("nothing started inside", plain), "",
              "kernel time of the chain %.1f us, span %.1f us" %
              (sum(t[3] for t in table) / 1e3, (table[-1][2] + table[-1][3] - table[0][2]) / 1e3), "",
              "| # | start us | dur us | gap us | queue | started inside the gap | kernel |", "|---|---|---|---|---|---|---|"]
    show = not since
    for i, name, s, d, gap, between, q in table:
        show = show or since in name
        if show:
            lines.append("| %d | %.1f | %.2f | %s | %s | %s | `%s` |" % (i, (s - t0) / 1e3, d / 1e3, "" if gap is None else "%.1f" % (gap / 1e3),
                                                                   q, ", ".join(between), short(name)))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:12]))


if __name__ == "__main__":
    main()
