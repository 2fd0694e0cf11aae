"""The owning device-buffer type (csrc/device_mem.h) on the host: tools/device_mem_main.cpp stands in for the allocation
point with malloc / free and walks DevBuf through alloc, reset, moves, upload, reserve, a failing allocation and release
after the context is gone.  Built here without a sanitizer; tools/device_mem_sanitize.sh builds the same program with
AddressSanitizer and UBSan."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_buffer_program(tmp_path):
    from raleigh_amd.build import CSRC
    exe = str(tmp_path / 'device_mem_main')
    cmd = [os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-O1', '-std=c++17', '-I', CSRC,
           os.path.join(ROOT, 'tools', 'device_mem_main.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all ok' in r.stdout
