#!/usr/bin/env python3
"""Writes tests/golden/traffic_types.json: the traffic types of the reference's experiment matrix, type name -> BASE_TRAFFIC_INTERVAL and
OTHER_CAR_SPEED, read from the reference's ``configs/*.json`` (settings only).

Usage: make_traffic_types.py <reference checkout>

The type of a config is in its file name: ``st_{t}``, ``train_{t}_{seed}``, ``combined_{t}_{seed}[b]`` run on traffic t;
``cross_{t1}_network_{t2}_traffic_{seed}[b]`` and ``ddpg_{t1}_network_{t2}_traffic_{seed}`` run a network trained on t1 on traffic t2.  The script
fails unless every config is one of these shapes, every config of a type agrees on the two fields, and both fields are present: all 86 configs
fall on the rows it writes."""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = (r"st_(?P<t>[a-z]+)", r"train_(?P<t>[a-z]+)_\d+", r"combined_(?P<t>[a-z]+)_\d+b?", r"cross_[a-z]+_network_(?P<t>[a-z]+)_traffic_\d+b?",
          r"ddpg_[a-z]+_network_(?P<t>[a-z]+)_traffic_\d+")


def main(reference):
    files = sorted(glob.glob(os.path.join(reference, "configs", "*.json")))
    rows, count = {}, 0
    for f in files:
        name = os.path.splitext(os.path.basename(f))[0]
        hit = [m for m in (re.fullmatch(s, name) for s in SHAPES) if m]
        assert len(hit) == 1, "config %s is none of the known shapes" % name
        cfg = json.load(open(f))
        row = {"BASE_TRAFFIC_INTERVAL": float(cfg["BASE_TRAFFIC_INTERVAL"]), "OTHER_CAR_SPEED": float(cfg["OTHER_CAR_SPEED"])}
        t = hit[0].group("t")
        assert rows.setdefault(t, row) == row, "config %s disagrees with the other %s configs: %r != %r" % (name, t, row, rows[t])
        count += 1
    assert count == len(files) == 86, "expected the reference's 86 configs, found %d" % len(files)
    out = os.path.join(HERE, "traffic_types.json")
    with open(out, "w") as fh:
        json.dump({t: rows[t] for t in sorted(rows)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d configs on %d rows -> %s" % (count, len(rows), out))
    for t in sorted(rows):
        print("  %-9s %r" % (t, rows[t]))


if __name__ == "__main__":
    main(sys.argv[1])
