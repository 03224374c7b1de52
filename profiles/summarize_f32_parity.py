"""f32_step_parity.txt (the lines tests/test_gpu_f32_step_parity.py appends to a GPU run's scratch output) -> the markdown
table of profiles/f32_step_parity.md: kernel / restatement per pipe, integrator, size and column, in units of 2^-24, the
worse of the column's two halves and of 1 and 4 ticks.  Usage: python profiles/summarize_f32_parity.py f32_step_parity.txt"""
import collections
import re
import sys

FIELDS = ("world_pos", "world_vel", "world_accel", "force")
CASE = re.compile(r"^(\S+) (rk4|semi_implicit) n (\d+) ticks (\d+): kernel (.*) \| restatement (.*)  \[2\^-24\]$")


def figures(text):
    t = text.split()
    return {t[i]: float(t[i + 1]) for i in range(0, len(t), 2)}


def main(path):
    rows, other = collections.OrderedDict(), []
    for line in open(path):
        m = CASE.match(line.rstrip("\n"))
        if not m:
            other.append(line.rstrip("\n"))
            continue
        cur = rows.setdefault((m.group(1), m.group(2), int(m.group(3))), {f: (0.0, 0.0) for f in FIELDS})
        k, r = figures(m.group(5)), figures(m.group(6))
        for f in FIELDS:
            cur[f] = (max(cur[f][0], k[f]), max(cur[f][1], r[f]))
    print("| pipe | integrator | n | " + " | ".join(f"{f} kernel / restatement" for f in FIELDS) + " |")
    print("|---|---|---|" + "---|" * len(FIELDS))
    worst = (0.0, None)
    for (pipe, integrator, n), c in rows.items():
        print(f"| {pipe} | {integrator} | {n} | " + " | ".join(f"{c[f][0]:.2f} / {c[f][1]:.2f}" for f in FIELDS) + " |")
        worst = max([worst] + [(c[f][0], (pipe, integrator, n, f)) for f in FIELDS], key=lambda w: w[0])
    print(f"\nworst kernel figure: {worst[0]:.2f} {worst[1]}\n")
    for line in other:       # the join, division-edge and poisoned-row cases, as the test wrote them
        if line:
            print("    " + line)


if __name__ == "__main__":
    main(sys.argv[1])
