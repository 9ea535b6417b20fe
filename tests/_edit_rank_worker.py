"""One rank of a several-process board for tests/test_gpu_edit.py (modelled on
_view_rank_worker.py): `python tests/_edit_rank_worker.py '<json>'` builds Engine.rank(...,
transport="ipc") as rank `rank` of `nranks`, runs load_random(seed) and step(turns), then pastes the
seeded random patterns `pastes` = [[x0, y0, w, h, op, pattern seed], ...] (not collective: the rows
this rank holds) -- every rank with only_holders false, else only a rank that holds rows of the
rectangle -- then step(more) and hash (both collective).  Prints one JSON line with the rank's rows,
the `changed` of every paste it made (None for one it skipped), the layouts written, the turn after
the pastes and the final hash."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]


def main():
    a = json.loads(sys.argv[1])
    import numpy as np

    import golhip
    r = a["rank"]
    e = golhip.Engine.rank(a["H"], a["W"], a["nranks"], r, bytes.fromhex(a["uid"]), device=a.get("device", 0),
                           transport="ipc")
    sh = e.shard(0)
    out = {"rank": r, "y0": sh["y0"], "y1": sh["y1"], "changed": [], "layouts": []}
    e.load_random(a["seed"])
    e.step(a["turns"])
    for x0, y0, w, h, op, seed in a["pastes"]:
        rows = {(y0 + j) % a["H"] for j in range(h)}
        if a["only_holders"] and not any(sh["y0"] <= y < sh["y1"] for y in rows):
            out["changed"].append(None)
            continue
        p = np.random.default_rng(seed).random((h, w)) < 0.5
        n, layout = e.paste(p, x0, y0, op, return_layout=True)
        out["changed"].append(n)
        out["layouts"].append(layout)
    out["turn"] = e.turn
    e.step(a["more"])
    out["hash"] = e.hash()
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
