"""One rank of a several-process board for tests/test_gpu_view.py (modelled on _rank_worker.py):
`python tests/_view_rank_worker.py '<json>'` builds Engine.rank(..., transport="ipc") as rank
`rank` of `nranks`, runs load_random(seed), step(turns) and view_counts(*view) (not collective: the
cells of this rank's rows), saves the frame to `out` (.npy) and prints one JSON line with the
rank's rows, the layout the frame was read from, the status of view() (pixels need every row
local) and the board hash (collective) after the views."""
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
    out = {"rank": r, "y0": sh["y0"], "y1": sh["y1"], "out": a["out"]}
    e.load_random(a["seed"])
    e.step(a["turns"])
    counts, layout = e.view_counts(*a["view"], return_layout=True)
    np.save(a["out"], counts)
    out["layout"] = layout
    try:
        e.view(*a["view"])
        out["view_error"] = 0
    except golhip.GolError as x:
        out["view_error"] = x.code
    out["hash"] = e.hash()
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
