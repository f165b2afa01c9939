"""Format the JSON lines tests/test_gpu_net_precision.py appends to $AO_PRECISION_REPORT as the table of a profiles/ note.

    AO_PRECISION_REPORT=precision.jsonl python -m pytest -m gpu tests/test_gpu_net_precision.py
    python tools/precision_table.py precision.jsonl > profiles/<name>.txt
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    from alpha_omok_amd.build import source_hash
    rows = [json.loads(l) for l in open(path) if l.strip()]
    print("source hash %s; %d cases; err = max over every board of the batch, against the float64 reference;" % (source_hash(), len(rows)))
    print("E32 = the float32 run of the same plain reference against its float64 run on the same boards (floor 1e-6)")
    print()
    print("%-22s %-28s %2s %2s %6s %5s %4s %5s | %8s %8s %7s | %8s %8s %7s | %4s | %8s %8s" % (
        "family", "kernel", "nb", "B", "planes", "batch", "mode", "w", "E32_l", "err_l", "err/E32", "E32_z", "err_z", "err/E32", "allw", "max dp", "max dv"))
    fam = {}
    for r in rows:
        print("%-22s %-28s %2d %2d %6d %5d %4d %5s | %8.2e %8.2e %7.2f | %8.2e %8.2e %7.2f | %4d | %8.1e %8.1e" % (
            r["family"], r["kernel"], r["nb"], r["B"], r["planes"], r["batch"], r["mode"], "fp16" if r["grid"] else "fp32",
            r["E32_l"], r["err_l"], r["ratio_l"], r["E32_z"], r["err_z"], r["ratio_z"], r["mult"], r["dp"], r["dv"]))
        f = fam.setdefault((r["family"], "fp16" if r["grid"] else "fp32", r["mult"]), [0.0, 0.0, 0])
        f[0], f[1], f[2] = max(f[0], r["ratio_l"]), max(f[1], r["ratio_z"]), f[2] + 1
    print()
    print("worst case per family:")
    print("%-22s %-5s %5s %12s %12s %8s" % ("family", "w", "cases", "logits / E32", "z / E32", "allowed"))
    for (name, w, mult), (a, b, n) in fam.items():
        print("%-22s %-5s %5d %12.2f %12.2f %8d" % (name, w, n, a, b, mult))


if __name__ == "__main__":
    main(sys.argv[1])
