"""One rank of a several-process board for tests/test_gpu_copy.py (modelled on
_edit_rank_worker.py): `python tests/_copy_rank_worker.py '<json>'` builds Engine.rank(...,
transport="ipc") as rank `rank` of `nranks`, runs load_random(seed) and step(turns), then for every
rectangle of `rects` = [[x0, y0, w, h], ...] reads copy_words and bounds (not collective: the rows
this rank holds), then cuts every rectangle of `cuts` of which it holds a row, then step(more) and
hash (both collective).  Prints one JSON line with the rank's rows, per rectangle the pattern words,
the alive count, the layout and the bounds, per cut the cells it cleared (None for one it skipped),
the turn after the reads and the final hash."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]


def main():
    a = json.loads(sys.argv[1])
    import golhip
    r = a["rank"]
    e = golhip.Engine.rank(a["H"], a["W"], a["nranks"], r, bytes.fromhex(a["uid"]), device=a.get("device", 0),
                           transport="ipc")
    sh = e.shard(0)
    out = {"rank": r, "y0": sh["y0"], "y1": sh["y1"], "copies": [], "cuts": []}
    e.load_random(a["seed"])
    e.step(a["turns"])
    for x0, y0, w, h in a["rects"]:
        words, alive, layout = e.copy_words(x0, y0, w, h, return_layout=True)
        out["copies"].append({"words": words.tolist(), "alive": alive, "layout": layout, "bounds": list(e.bounds(x0, y0, w, h))})
    out["turn"] = e.turn
    for x0, y0, w, h in a["cuts"]:
        rows = {(y0 + j) % a["H"] for j in range(h)}
        if not any(sh["y0"] <= y < sh["y1"] for y in rows):
            out["cuts"].append(None)
            continue
        out["cuts"].append(e.copy_words(x0, y0, w, h, cut=True)[1])
    e.step(a["more"])
    out["hash"] = e.hash()
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
