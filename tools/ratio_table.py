"""Dev tool: condense the output of

    python -m pytest tests/test_gpu_aggregate_train.py -q -s > LOG

into profiles/aggregate_train_ratios.txt.  The run prints one RATIO line per (path, case,
tensor) -- err, e_o32, max|g64| and err / noise -- some 5 700 of them; the table keeps every
err / noise as one row per (path, case) with one column per tensor, and copies the run's
WORST, GROUP and d_p1 lines and the SIGNS lines with a nonzero count as they stand.

    python tools/ratio_table.py LOG > profiles/aggregate_train_ratios.txt
"""
import collections
import re
import sys

LINE = re.compile(r"RATIO (\S+)\s+(\S+)\s+(.+?)\s+err \S+\s+e_o32 \S+\s+max\|g64\| \S+\s+err/noise\s+(\S+)")
SHORT = (("d color_branch.", "dC"), ("d alpha_branch.0.", "dA."), ("d block", "dB"), (".weight", ".w"), (".bias", ".b"),
         ("dconf_pair", "dcf_pair"), ("feat ", "f."), ("d ", "d_"), ("colour", "col"))


def short(t):
    for a, b in SHORT:
        t = t.replace(a, b)
    return t


def main(log):
    rat, cols = collections.OrderedDict(), collections.OrderedDict()   # path -> case -> tensor -> ratio
    worst, extra, signs = [], [], []
    for ln in open(log):
        for tag, keep in (("WORST ", worst), ("GROUP ", extra), ("SIGNS ", signs)):
            at = ln.find(tag)
            if at >= 0 and not (tag == "SIGNS " and " 0 of " in ln):
                keep.append(ln[at:].rstrip("\n"))
        at = ln.find("RATIO ")
        if at < 0:
            continue
        ln = ln[at:].rstrip("\n")
        path, case, tensor, r = LINE.match(ln).groups()
        if tensor.startswith("d_p1"):           # the atomic d_p1 check: two lines per case, kept whole
            extra.insert(len([x for x in extra if x.startswith("RATIO")]), ln)
            continue
        d = rat.setdefault(path, collections.OrderedDict()).setdefault(case, {})
        d[tensor] = max(float(r), d.get(tensor, -1.0))   # a case that ran twice: the larger
        cols.setdefault(tensor, None)
    cols = list(cols)
    out = ["err / max(e_o32, 2^-22 max|g64|) of tests/test_gpu_aggregate_train.py on one MI355X: every (path, case, tensor) of the run,",
           "one row per (path, case), one column per tensor ('-': the case has no such tensor on that path); then the WORST table",
           "of the run, the atomic d_p1 check, the grouping time and the saved signs that differ from z64 > 0.",
           "Made by tools/ratio_table.py from the run's pytest -s output (its RATIO lines also give err, e_o32 and max|g64|).",
           "columns: " + ", ".join(f"{short(t)} = {t}" for t in cols), ""]
    for path, cases in rat.items():
        out.append(f"{'RATIO ' + path:26s}" + "".join(f"{short(t):>9s}" for t in cols))
        for case, d in cases.items():
            out.append(f"{path + ' ' + case:26s}" + "".join(f"{d[t]:9.2f}" if t in d else f"{'-':>9s}" for t in cols))
        out.append("")
    out += worst + [""] + extra + ["", "Saved signs that differ from z64 > 0 (every other layer of every run: 0), all within their bar"]
    print("\n".join(out + signs))


if __name__ == "__main__":
    main(sys.argv[1])
