"""Camera-ray launches of a one-pipe frame, from rocprofv3 output:
  python tools/camera_launches.py KERNEL_TRACE.csv [COUNTER_COLLECTION.csv] [--rays N]
A camera launch is the first closest-hit launch after a k_camera launch (one
pipe: launches run in enqueue order), whichever kernel serves it
(k_trace_closest or k_trace_camera). Prints their count, mean and maximum
time, the other closest-hit launches' and -- given a counter file -- each
counter's sum over the camera launches, per camera ray with --rays (camera
rays of the frame)."""
import argparse
import csv
import json
import re


def short(name):
    m = re.search(r"(k_\w+?)(E|\(|<|$)", name)
    return m.group(1) if m else name


def camera_flags(rows, key):
    """rows in dispatch order -> the dispatch ids of camera launches / other closest-hit launches"""
    cam, other, armed = [], [], False
    for r in rows:
        k = short(r["Kernel_Name"])
        if k.startswith("k_camera"):
            armed = True
        elif k.startswith(("k_trace_closest", "k_trace_camera")):
            (cam if armed else other).append(r[key])
            armed = False
    return cam, other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("counters", nargs="?")
    ap.add_argument("--rays", type=float, default=0.0)
    a = ap.parse_args()
    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    ms = {r["Dispatch_Id"]: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows}
    cam, other = camera_flags(rows, "Dispatch_Id")
    out = {}
    for name, ids in (("camera", cam), ("other_closest", other)):
        t = [ms[i] for i in ids]
        out[name] = {"launches": len(t), "total_ms": round(sum(t), 3), "mean_ms": round(sum(t) / max(1, len(t)), 4),
                     "max_ms": round(max(t), 4) if t else 0.0}
    out["all_kernels_ms"] = round(sum(ms.values()), 3)
    if a.counters:
        crow = list(csv.DictReader(open(a.counters)))
        disp = {}
        for r in crow:  # one row per dispatch and counter
            disp.setdefault(int(r["Dispatch_Id"]), {"Kernel_Name": r["Kernel_Name"], "c": {}})["c"][r["Counter_Name"]] = \
                float(r["Counter_Value"])
        order = [dict(Kernel_Name=disp[i]["Kernel_Name"], id=i) for i in sorted(disp)]
        ccam, _ = camera_flags(order, "id")
        sums = {}
        for i in ccam:
            for k, v in disp[i]["c"].items():
                sums[k] = sums.get(k, 0.0) + v
        out["camera_counters"] = {"launches": len(ccam), **{k: v for k, v in sorted(sums.items())}}
        if a.rays:
            out["camera_counters_per_ray"] = {k: round(v / a.rays, 3) for k, v in sorted(sums.items())}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
