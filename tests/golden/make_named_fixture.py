"""Regenerates tests/golden/wb5_named_24.json: the first 24 boards of the reference's data file wb5/dataset_for_vs_wb5.json,
as they are (DATA only).  Run where the reference is present: python tests/golden/make_named_fixture.py [path to the json]"""
import json, os, sys  # noqa: E401

json.dump({"logs": json.load(open(sys.argv[1] if len(sys.argv) > 1 else "/root/reference/wb5/dataset_for_vs_wb5.json"))["logs"][:24]}, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "wb5_named_24.json"), "w"))
