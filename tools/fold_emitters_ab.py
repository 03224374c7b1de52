#!/usr/bin/env python3
"""Do two commits generate the same fold kernels?  (profiles/fold_emitters_refactor.md)

A corpus of programs with fold stages — hand-written folds and whole-world StableHLO modules, baked / device / complete-graph
edges, with and without gather_batch, wave kernels, direct output and replicas, plus the stand-alone fold — is generated with
codegen.generate_source(tp, "float64", 2) at a parent revision (`git archive` of it, unpacked into a temporary directory) and
in this tree.  An entry passes when the two texts are byte-identical, or when they are the same code: both built with
codegen.build, disassembled with isa_check.disassemble, and the instruction text of every fold*_kernel / fold*_wave /
fold*_commit equal once addresses and symbol hashes are taken out.  Every differing text line is printed, so a change outside
the fold kernels (a comment, the launch entry) is seen and can be given its reason.  No GPU is needed.

    python tools/fold_emitters_ab.py [--parent HEAD]
"""
import argparse
import difflib
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FOLD_SYMBOL = re.compile(r"fold\d+_(kernel|wave|commit)|graph_fold_(kernel|commit)")


def corpus():
    """[(entry name, thunk -> generated text, thunk -> built .so)]: a fresh Program (and world_program result) per entry —
    a Program caches its first trace."""
    from elodin_amd import codegen, dsl, stablehlo as sh
    from tests import fold_tables_common as ft, test_program_folds_host as pf
    from tests.golden import hlo_world_builder as hb
    out = []

    def add(name, make_tp):
        out.append((name, lambda: codegen.generate_source(make_tp(), "float64", 2), lambda: codegen.build(make_tp(), "float64", 2)))

    def hand(name, prog, widths, edges, tables=("baked", "device"), **kw):
        for t in tables:
            add(f"{name}/{t}", lambda t=t: prog().trace(widths, fold_edges={"e": edges}, fold_tables=t, **kw))

    chain = lambda: dsl.Program([pf.double, pf.fold_test, pf.add_one], dsl.pipe(), [])
    hand("chain", chain, {"x": 1, "n": 1}, pf.EDGES["e"])
    hand("chain-replicas-5x3", chain, {"x": 1, "n": 1}, pf.EDGES["e"], fold_replicas=(5, 3))
    hand("sum-wave", lambda: ft.sum_program(True), {"x": 1, "y": 1, "z": 1}, pf.EDGES["e"])
    hand("sum-seq", lambda: ft.sum_program(False), {"x": 1, "y": 1, "z": 1}, pf.EDGES["e"])
    hand("damped", ft.damped_program, {"x": 1, "y": 1, "z": 1}, pf.EDGES["e"], tables=("device",))
    hand("sum-seq-complete128", lambda: ft.sum_program(False), {"x": 1, "y": 1, "z": 1}, ("complete", 128), tables=("device",))

    def world(name, module, **kw):
        for t in ("baked", "device"):
            def make_tp(t=t):
                prog, manifest, edges = sh.world_program(*module(), **kw)
                return prog.trace({c["column"]: c["width"] for c in manifest["columns"]}, fold_edges=edges, fold_tables=t)
            add(f"{name}/{t}", make_tp)

    ring = lambda ks: {s_: [(s_ + k) % 70 for k in ks] for s_ in range(70)}
    world("nbody72-waves", lambda: hb.nbody_world(72, 2.9591220828e-4, 1e-6), wave_folds=True)
    world("nbody72-sequential", lambda: hb.nbody_world(72, 2.9591220828e-4, 1e-6), wave_folds=False)
    world("edges70x3", lambda: hb.edge_fold_world(70, ring((1, 5, 11)), "newton", (6.6743e-11,)))
    world("edges70x5", lambda: hb.edge_fold_world(70, ring((1, 5, 11, 17, 23)), "newton", (6.6743e-11,)))
    world("edges70x64-waves", lambda: hb.edge_fold_world(70, ring(range(1, 65)), "newton", (6.6743e-11,)), wave_folds=True)
    out.append(("standalone/fold_test", lambda: codegen.generate_graph_fold_source(pf.fold_test.trace({"x": 1})),
                lambda: codegen.build_graph_fold(pf.fold_test.trace({"x": 1}))))
    return out


def fold_kernels(so):
    """{demangled-enough symbol: instruction text} of the fold kernels of a built object: addresses, the offsets objdump prints
    after a symbol and symbol hashes removed."""
    from elodin_amd import isa_check
    got = {}
    for name, lines in isa_check.kernels(isa_check.disassemble(Path(so))).items():
        m = FOLD_SYMBOL.search(name)
        if m and any(ln.strip().startswith("s_endpgm") for ln in lines):
            text = "\n".join(re.sub(r"\s*//.*$", "", ln).strip() for ln in lines)
            got[m.group(0)] = re.sub(r"_Z\w+", "<sym>", text)
    return got


def emit(out_dir, build):
    """Child mode, run with a tree's own elodin_amd on the path: the texts, and the fold kernels' instructions of `build`."""
    out_dir = Path(out_dir)
    for name, text, so in corpus():
        stem = name.replace("/", "__")
        (out_dir / f"{stem}.cpp").write_text(text())
        if name in build:
            (out_dir / f"{stem}.isa.json").write_text(json.dumps(fold_kernels(so())))


def run_emit(tree, out_dir, build=()):
    env = dict(os.environ, PYTHONPATH=str(tree))
    subprocess.run([sys.executable, str(Path(__file__).resolve()), "--emit", str(out_dir), "--build", ",".join(build)],
                   cwd=tree, env=env, check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--emit", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--build", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.emit:
        sys.path.insert(0, os.getcwd())
        return emit(a.emit, set(filter(None, a.build.split(","))))
    with tempfile.TemporaryDirectory() as t:
        old_tree, old, new = Path(t, "parent"), Path(t, "old"), Path(t, "new")
        for d in (old_tree, old, new):
            d.mkdir()
        rev = subprocess.run(["git", "rev-parse", "--short", a.parent], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
        tar = subprocess.run(["git", "archive", a.parent], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(old_tree)], input=tar, check=True)
        run_emit(old_tree, old)
        run_emit(ROOT, new)
        names = sorted(p.name[:-4] for p in new.glob("*.cpp"))
        differ = [n.replace("__", "/") for n in names if (old / f"{n}.cpp").read_bytes() != (new / f"{n}.cpp").read_bytes()]
        if differ:      # same code?  build both, compare the fold kernels' instructions
            run_emit(old_tree, old, differ)
            run_emit(ROOT, new, differ)
        rows, notes, ok = [], [], True
        for n in names:
            a_, b_ = (old / f"{n}.cpp").read_text(), (new / f"{n}.cpp").read_text()
            sha = lambda s: hashlib.sha256(s.encode()).hexdigest()[:16]
            if a_ == b_:
                verdict = "text identical"
            else:
                ka, kb = json.loads((old / f"{n}.isa.json").read_text()), json.loads((new / f"{n}.isa.json").read_text())
                per = {k: ("same instructions" if ka.get(k) == kb.get(k) else "DIFFERENT") for k in sorted(set(ka) | set(kb))}
                ok &= bool(per) and all(v == "same instructions" for v in per.values())
                verdict = "; ".join(f"`{k}` {v}" for k, v in per.items())
                changed = [ln for ln in difflib.unified_diff(a_.splitlines(), b_.splitlines(), "parent", "new", lineterm="", n=0)
                           if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
                notes.append(f"### {n.replace('__', '/')}\n\n```diff\n" + "\n".join(changed) + "\n```\n")
            rows.append(f"| `{n.replace('__', '/')}` | `{sha(a_)}` | `{sha(b_)}` | {verdict} |")
        table = (f"| entry | sha256 at {rev} (first 16) | sha256 new (first 16) | verdict |\n|---|---|---|---|\n" + "\n".join(rows) + "\n\n" +
                 (("## Text lines that differ\n\n" + "\n".join(notes)) if notes else "No text line differs in any entry.\n"))
        print(table)
        sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
