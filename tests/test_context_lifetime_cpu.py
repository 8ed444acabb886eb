"""What a context reserves from the runtime -- device memory, pinned memory, events -- against a counting fake of the HIP
runtime, on the CPU, under AddressSanitizer + UBSan + LeakSanitizer.

csrc/adsb_context.cpp (create, destroy, the registry and every lazy reservation), adsb_ring.cpp,
adsb_decim.cpp and adsb_replay_host.cpp are compiled as they are by g++ and linked with tests/context_fake_hip.cpp: the
fake runtime (live sets, abort on a free of what is not live, poisoned fresh memory, "the n-th call from now fails"), stubs
for the launches below those units, and the driver.  The driver asserts, for a context of one buffer and one of 17 (the
smallest that scores on the device):

1. with everything reserved that can be (signal statistics, receivers 1 then 2 with receiver scoring, a CS16 ring in one
   context and a CU8 ring in another, the fallback lists, both stagings grown, the address and key lists grown, the CU8
   widen buffer, shard lists with and without the fresh list, a registered host range, a decimator handle whose staging
   has grown) adsb_destroy leaves only the pool's streams live;
2. adsb_create with its n-th runtime call failing, for every n up to the number a successful one makes: an error, *out
   null, the live set as before, and a following unarmed adsb_create succeeds (a small context's pool streams are made
   first: the pool tolerates a refused CU mask by design, so that failure is none of adsb_create's);
3. every lazy reservation (ensure_signal_stats, ensure_rx_scoring, ensure_fallback, ensure_shard_lists, the ring of
   either format, adsb_decim_create) with its n-th runtime call failing, for every n: an error and the live set as
   before.  A deliberate deviation from "an unarmed retry after every failure": the retry is the next ARMED attempt in
   the same context, which has to get past the call that failed before, and only the last attempt is unarmed.  A retry
   that skips work ends before its armed call and then fails the check that follows: every slot's views of the feature
   non-null -- for receiver scoring rx_map, first, rx_slot and out_add_rx of every slot, for the shard lists h_fresh,
   d_fresh_seen and h_earlier.  A second deviation: the growers (the two stagings, the address and key lists, the keyed
   sets re-made for another number of receivers) release the old buffer before they reserve the new one, as they always
   did, so that the two never add up; their failure leaves the live set one buffer short -- not equal -- the view null
   and the size zero, and the retry succeeds;
4. a context created, used for nothing and destroyed releases exactly what it reserved.

No GPU.  The same features are held to the oracle on the device by the GPU suite."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.conftest import ROOT

CSRC = ROOT / "dump1090_rs_amd" / "csrc"
UNITS = ["adsb_context.cpp", "adsb_ring.cpp", "adsb_decim.cpp", "adsb_replay_host.cpp"]
SOURCES = [ROOT / "tests" / "context_fake_hip.cpp", *(CSRC / u for u in UNITS)]
HIP_INCLUDE = Path("/opt/rocm/include")
EXE = ROOT / "tests" / "context_lifetime_asan"


def have(lib: str) -> bool:
    if shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime.h").exists():
        return False
    p = subprocess.run(["gcc", f"-print-file-name={lib}"], capture_output=True, text=True).stdout.strip()
    return bool(p) and Path(p).exists()


def build() -> Path:
    deps = [*SOURCES, *CSRC.glob("*.h"), *CSRC.glob("*.hpp"), ROOT / "include" / "adsb_hip.h"]
    if EXE.exists() and EXE.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return EXE
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}",
                    *map(str, SOURCES), "-o", str(EXE)], check=True)
    return EXE


def test_context_lifetime_against_counting_fake_runtime():
    if not have("libasan.so"):
        pytest.skip("no libasan / g++ / HIP headers in this environment")
    exe = build()
    limit = "ulimit -t 60; exec \"$0\""   # a minute of CPU time at the most
    r = subprocess.run(["sh", "-c", limit, str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "context lifetime ok:" in r.stdout, r.stdout[-1500:] + r.stderr[-6000:]
    for word in ("AddressSanitizer", "LeakSanitizer", "runtime error", "fake HIP:"):
        assert word not in r.stderr, r.stderr[-6000:]
    words = r.stdout.split("context lifetime ok:")[1].split()
    # the run did what it is for: adsb_create's sweeps were as long as a context's reservations are many, and the lazy
    # reservations were failed often enough to have reached every call of each
    assert int(words[words.index("checks;") - 1]) >= 1000
    assert int(words[words.index("large,") - 1]) >= 100 and int(words[words.index("small;") - 1]) >= 100
    assert int(words[words.index("lazy-reservation") - 1]) >= 100
