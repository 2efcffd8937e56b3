"""The conv Q-network's host-side layout (dronerl_amd/csrc/convnet/
dronerl_convnet_layout.h: map sides, K and N padding, offsets inside the
packed image, the element -> parameter map, the folded flatten, the LDS plan)
checked by a stand-alone program under the address and undefined-behaviour
sanitizers: tests/native/convnet_layout_check.cpp.  Nothing is loaded into
Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_convnet_layout_maps_every_parameter_once(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "convnet_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(os.path.dirname(HERE), "include"),
                    "-o", exe, os.path.join(HERE, "native", "convnet_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
