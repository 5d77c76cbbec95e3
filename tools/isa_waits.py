"""In-order wait model of a kernel's step loop in a hipcc -S listing: how many
cycles a lone wave stalls on LDS (lgkmcnt) latency that nothing hides.

    python tools/isa_waits.py <file.s> <kernel-symbol-regex> [L=128] [n_loops=1]

The model walks the largest loop(s) of the function linearly (inner branches
are ignored).  Every VALU / MFMA / LDS / VMEM instruction costs 4 issue cycles,
every SALU one.  LDS instructions and scalar loads enter the lgkm queue at their
issue time; at `s_waitcnt lgkmcnt(N)` the wave stalls until every queued entry
but the newest N is L cycles old (LDS returns in order).  It prints, per loop:
issue cycles, the number of lgkmcnt waits, how many of them come within five
instructions of the last ds_read, and the exposed (stalled) cycles.

L is an assumption, not a measured latency: the model ranks schedules of the
same loop against each other; it knows nothing of MFMA result
latency, VMEM, bank conflicts or a second wave on the SIMD."""
import re
import sys


def function_body(lines, pat):
    start = next(i for i, l in enumerate(lines)
                 if re.match(r"^\S+:", l) and not l.startswith(".") and pat.search(l.split(":")[0]))
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def largest_loops(body, n):
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_(?:c)?branch\w*\s+(\.LBB\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    loops.sort(key=lambda x: x[0] - x[1])
    shown = []
    for lo, hi in loops:
        if any(lo >= a and hi <= b for a, b in shown):
            continue
        shown.append((lo, hi))
        if len(shown) == n:
            break
    return shown


def instructions(body, lo, hi):
    for l in body[lo:hi + 1]:
        l = l.split(";")[0].strip()
        if not l or l[0] == "." or l.endswith(":"):
            continue
        yield l


def model(insts, L):
    """-> (instructions, issue cycles, lgkmcnt waits, waits near a ds_read, exposed cycles)"""
    t = issue = exposed = waits = near = n = 0
    queue = []  # issue times of the outstanding lgkm operations, oldest first
    since_read = None  # instructions since the last ds_read
    for ins in insts:
        op = ins.split()[0]
        n += 1
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                waits += 1
                if since_read is not None and since_read <= 5:
                    near += 1
                cut = len(queue) - min(int(m.group(1)), len(queue))
                if cut:
                    ready = queue[cut - 1] + L
                    if ready > t:
                        exposed += ready - t
                        t = ready
                queue = queue[cut:]
        cost = 1 if op.startswith("s_") else 4
        if op.startswith("ds_") or op.startswith(("s_load", "s_buffer_load")):
            queue.append(t)
        if op.startswith("ds_read") or op.startswith("ds_load"):
            since_read = 0
        elif since_read is not None:
            since_read += 1
        t += cost
        issue += cost
    return n, issue, waits, near, exposed


def main():
    path, pat = sys.argv[1], re.compile(sys.argv[2])
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    nl = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    body = function_body(open(path).read().split("\n"), pat)
    print(body[0][:150])
    for lo, hi in largest_loops(body, nl):
        n, issue, waits, near, exposed = model(instructions(body, lo, hi), L)
        print(f"loop lines {lo}-{hi}: {n} instructions, {issue} issue cycles, {waits} lgkmcnt waits "
              f"({near} within 5 instructions of the last ds_read), exposed {exposed} cycles at L={L} "
              f"-> {issue / (issue + exposed):.2f} issue-active")


if __name__ == "__main__":
    main()
