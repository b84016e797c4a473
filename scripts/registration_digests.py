"""One SHA-256 per array that the ragged-batch entries return, on the inputs of tests/registration_cases.py: the registration
entries, probabilistic_sample_batch, chamfer_batch, voxel_down_sample_batch and crop_batch, each for numpy, device and mixed
inputs.  The algorithms are deterministic, so two checkouts that load the same library must print the same lines; a line
that differs is a marshalling bug.

    python scripts/registration_digests.py [--package DIR] [--out FILE] [--record-calls FILE]

--package DIR imports pcrcg_amd from DIR (another checkout, with its built library) and not from this one; the cases always
come from this checkout.  --record-calls FILE also writes what tests/test_registration_calls_gpu.py compares with: the
library calls of every case, after checking that the three forms of input give one record.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", default=REPO)
    ap.add_argument("--out")
    ap.add_argument("--record-calls")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from tests import registration_cases as RC
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    import pcrcg_amd
    dev = torch.device("cuda", 0)
    lines = [f"# pcrcg_amd from {os.path.relpath(os.path.dirname(pcrcg_amd.__file__), REPO)}"]
    for form in RC.FORMS:
        for name, call in RC.cases(form, dev):
            lines += [f"{form} {name}{path} {digest}" for path, digest in RC.digests(call())]
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    if args.record_calls:
        records = [RC.record_calls(form, dev) for form in RC.FORMS]
        same = [json.dumps(r) == json.dumps(records[0]) for r in records]
        if not all(same):
            sys.exit(f"the forms {RC.FORMS} do not give one record: {same}")
        with open(args.record_calls, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in records[0].items()) + "\n}\n")
        print(f"# {sum(len(v['calls']) for v in records[0].values())} calls of {len(records[0])} cases -> {args.record_calls}")


if __name__ == "__main__":
    main()
