"""Generates tests/golden/g1_effort_limits.json: the actuated joints of the reference's MuJoCo model of the G1 and the magnitude of their
actuatorfrcrange [N m], in the order of the file.  Data recorded from the reference's model file; run where that file is:

    python tests/golden/make_effort_limits_golden.py PATH/robot_models/unitree_g1/g1_description/urdf/g1_29dof.xml
"""
import json
import os
import sys
import xml.etree.ElementTree as ET

limits = {}
for j in ET.parse(sys.argv[1]).getroot().iter("joint"):
    if "actuatorfrcrange" in j.attrib:
        lo, hi = (float(v) for v in j.attrib["actuatorfrcrange"].split())
        assert -lo == hi > 0.0, j.attrib
        limits[j.attrib["name"]] = hi
assert len(limits) == 29, len(limits)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "g1_effort_limits.json"), "w") as f:
    json.dump(limits, f, indent=1)
    f.write("\n")
