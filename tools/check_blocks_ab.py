#!/usr/bin/env python3
"""tools/check_blocks_bench.py of two builds, alternating, merged into one record.

    check_blocks_ab.py PARENT_TREE [--passes N] [--out FILE] [-- bench options]

PARENT_TREE is a built checkout of the parent commit (its own package, library
and tools); the other build is the tree this script lies in.  Each pass runs
the parent's bench and then this tree's, each in a process of its own, so
neither build is favoured by what the other left warm; the seconds of
Context.check_blocks on the complete trees ("complete") and of the C call
("complete_c") go to profiles/load_blocks/check_blocks_ab.json with, per
build, min, median and max over all passes.  The criterion recorded per case:
the median of the new build's runs lies inside the parent's min-max band.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("complete", "complete_c")


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "load_blocks", "check_blocks_ab.json"))
    a = ap.parse_args(argv)
    trees = {"parent": os.path.abspath(a.parent), "new": ROOT}
    passes = {side: [] for side in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for p in range(a.passes):
            for side, tree in trees.items():
                out = os.path.join(tmp, "%s%d.json" % (side, p))
                env = {k: v for k, v in os.environ.items()
                       if k not in ("PYTHONPATH", "CIRUELA_AMD_LIB")}
                subprocess.run([sys.executable, os.path.join(tree, "tools", "check_blocks_bench.py"),
                                "--out", out] + extra, check=True, cwd=tree, env=env)
                with open(out) as f:
                    passes[side].append(json.load(f))
    result = {"what": "tools/check_blocks_bench.py%s, the parent commit's build and this one "
                      "alternated %d times on one MI355X, each run a process of its own; seconds "
                      "per run" % ("".join(" " + e for e in extra), a.passes),
              "criterion": "the median of the new build's runs lies inside the parent's own "
                           "min-max band",
              "cases": {}}
    for case in passes["new"][0]["cases"]:
        rec = {}
        for m in METHODS:
            rec[m] = {}
            for side in trees:
                runs = [r["cases"][case]["methods"][m]["seconds"] for r in passes[side]]
                flat = [s for r in runs for s in r]
                rec[m][side] = {"passes": runs, "min": min(flat), "median": median(flat),
                                "max": max(flat)}
            rec[m]["inside"] = rec[m]["parent"]["min"] <= rec[m]["new"]["median"] <= \
                rec[m]["parent"]["max"]
            rec[m]["new_over_parent_median"] = rec[m]["new"]["median"] / rec[m]["parent"]["median"]
        one = passes["new"][0]["cases"][case]
        rec.update(files=one["files"], bytes=one["bytes"], blocks=one["blocks"])
        result["cases"][case] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({c: {m: [round(r[m][s]["median"], 4) for s in trees] + [r[m]["inside"]]
                          for m in METHODS} for c, r in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
