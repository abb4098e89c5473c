"""Dev tool: instruction counts of one kernel in hipcc's device assembly
(`hipcc ... --cuda-device-only -S`), for the whole kernel and for the tile loops of a
producer / consumer kernel.  Usage: tools/asm_counts.py file.s kernel_name_substring

A loop is taken from a backward branch: label .LBBn_m up to a branch back to it.
Per tile loop it prints the lane-move, load, LDS-read, wait and barrier counts,
and with --window A B the same between the A-th and B-th barrier of the producer
loop in program order (counted from 0; block placement need not follow the
schedule, so check the printed barrier lines against the source)."""
import argparse
import re


def kernel_lines(path, name):
    out, on = [], False
    for line in open(path):
        if not on and re.match(r"^\S*%s\S*:\s" % re.escape(name), line) and ".kd" not in line:
            on = True
            continue
        if on:
            if line.startswith(".Lfunc_end"):
                break
            out.append(line.rstrip("\n"))
    return out


def count(lines):
    pat = {"readlane": r"\bv_readlane_b32", "writelane": r"\bv_writelane_b32", "readfirstlane": r"\bv_readfirstlane_b32",
           "global_load": r"\bglobal_load_", "buffer_load": r"\bbuffer_load_", "ds_read": r"\bds_read", "s_load": r"\bs_load_",
           "s_waitcnt": r"\bs_waitcnt", "s_barrier": r"\bs_barrier", "s_nop": r"\bs_nop", "branch": r"\bs_cbranch|\bs_branch",
           "mfma": r"\bv_mfma", "valu": r"^\s+v_(?!mfma)"}
    return {k: sum(1 for ln in lines if re.search(p, ln)) for k, p in pat.items()}


def spans(lines):
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label[m.group(1)] = i
    out = []
    for i, ln in enumerate(lines):
        m = re.search(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in label and label[m.group(1)] <= i:
            out.append((label[m.group(1)], i))
    return out


def tile_loops(lines):
    """(producer, consumer) line ranges: the union of the backward-branch spans
    that hold barriers and no MFMA, and the smallest span that holds every MFMA
    (block placement can wrap one more span around both; that one is neither)."""
    has = lambda a, b, pat: any(re.search(pat, ln) for ln in lines[a:b + 1])
    mf = [i for i, ln in enumerate(lines) if re.search(r"\bv_mfma", ln)]
    sp = spans(lines)
    prod = [(a, b) for a, b in sp if has(a, b, r"\bs_barrier") and not has(a, b, r"\bv_mfma")]
    cons = [(a, b) for a, b in sp if mf and a <= mf[0] and mf[-1] <= b]
    p = (min(a for a, _ in prod), max(b for _, b in prod)) if prod else None
    c = min(cons, key=lambda ab: ab[1] - ab[0]) if cons else None
    return p, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--window", type=int, nargs=2, default=None)
    a = ap.parse_args()
    ls = kernel_lines(a.asm, a.kernel)
    print("kernel", a.kernel, "lines", len(ls), count(ls))
    for what, rng in zip(("producer loop", "consumer loop"), tile_loops(ls)):
        if rng is None:
            continue
        body = ls[rng[0]:rng[1] + 1]
        print("  %s lines %d..%d" % (what, rng[0], rng[1]), count(body))
        if a.window and what == "producer loop":
            bars = [i for i, ln in enumerate(body) if re.search(r"\bs_barrier", ln)]
            print("    barriers at", bars)
            if len(bars) > a.window[1]:
                print("    between barrier %d and %d:" % tuple(a.window), count(body[bars[a.window[0]]:bars[a.window[1]]]))


if __name__ == "__main__":
    main()
