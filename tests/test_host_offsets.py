"""CPU: the host layer's index arithmetic (cess_amd/csrc/host_pure.hpp: message
offset staging, shard ranges, bitmap words) built into a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer.  The header needs no HIP,
so the same code the host APIs run is checked here without a GPU; the driver
(tests/hostemu/host_offsets_main.cpp) holds the cases."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_offsets_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_offsets")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostemu", "host_offsets_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "OK: host offsets, shards, bitmap" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
