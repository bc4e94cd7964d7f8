"""Records the function signatures of the reference's tools.py in tests/golden/reference_signatures_tools.json, in the format
of reference_signatures.json: {"tools": {name: [[parameter, default or "<required>"], ...]}}.  The module imports xarray
and dask, which need not be installed: the source is parsed with ast, not imported.

    python tests/golden/make_tools_signatures.py <reference checkout>/src/das4whales/tools.py"""
import ast
import json
import os
import sys


def signatures(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    out = {}
    for node in tree.body:
        if not isinstance(node, ast.FunctionDef):
            continue
        a = node.args
        pos = a.posonlyargs + a.args
        defaults = ["<required>"] * (len(pos) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
        params = [[p.arg, d] for p, d in zip(pos, defaults)]
        params += [[p.arg, "<required>" if d is None else ast.literal_eval(d)] for p, d in zip(a.kwonlyargs, a.kw_defaults)]
        if a.vararg:
            params.append([a.vararg.arg, "<required>"])
        if a.kwarg:
            params.append([a.kwarg.arg, "<required>"])
        out[node.name] = params
    return out


if __name__ == "__main__":
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_signatures_tools.json")
    with open(dst, "w") as f:
        json.dump({"tools": signatures(sys.argv[1])}, f, indent=1, sort_keys=True)
        f.write("\n")
