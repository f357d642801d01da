"""CPU: the two libraries csrc/build.sh leaves behind, and csrc/tuning.h's perturbed-schedule switches at their defaults.

The perturbed-schedule variant (libmsae_hip_perturb.so; tests/test_gpu_perturbed_schedule.py runs the fused encoder on it)
exports the probes' msae_perturb_* functions; the PRODUCT must not contain them, and with neither switch defined tuning.h gives
probe macros that expand to nothing -- their arguments are not even evaluated -- and a grid cap that is the identity.
"""
import shutil
import struct
import subprocess

from conftest import REPO

LIB_DIR = REPO / "multimodal-sae_amd" / "msae" / "_lib"
CSRC = REPO / "multimodal-sae_amd" / "csrc"
PERTURB_EXPORTS = {"msae_perturb_set_seed", "msae_perturb_reset", "msae_perturb_hits", "msae_perturb_site_name",
                   "msae_perturb_launches"}
BUILD_HINT = "build both libraries with `sh multimodal-sae_amd/csrc/build.sh` (python __graft_entry__.py)"


def _exported(path):
    """Names of the defined global / weak symbols of an ELF64 little-endian shared object's .dynsym (no tool, no dlopen)."""
    data = path.read_bytes()
    assert data[:6] == b"\x7fELF\x02\x01", f"{path}: not a 64-bit little-endian ELF file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:                                 # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for s in range(off, off + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", data, s)
            if st_shndx != 0 and (st_info >> 4) in (1, 2):    # defined; STB_GLOBAL or STB_WEAK
                end = data.index(b"\0", str_off + st_name)
                names.add(data[str_off + st_name:end].decode())
    return names


def test_only_the_variant_exports_the_probe_functions():
    product, variant = LIB_DIR / "libmsae_hip.so", LIB_DIR / "libmsae_hip_perturb.so"
    assert product.exists() and variant.exists(), f"{product} or {variant} is missing: {BUILD_HINT}"
    p, v = _exported(product), _exported(variant)
    assert "msae_encode_topk" in p and "msae_abi_version" in p, "the .dynsym reader found no product symbol"
    assert not [n for n in p if n.startswith("msae_perturb")], "the product library exports probe functions"
    assert b"msae_perturb_" not in product.read_bytes(), "the product library contains a probe function's name"
    assert PERTURB_EXPORTS <= v, f"the variant does not export {sorted(PERTURB_EXPORTS - v)}"
    # everything else is the same C ABI
    assert {n for n in p if n.startswith("msae_")} == {n for n in v if n.startswith("msae_")} - PERTURB_EXPORTS


HOST_PROGRAM = r"""
#include "tuning.h"
#ifdef MSAE_PERTURB
#error "MSAE_PERTURB is defined without a -D"
#endif
static_assert(MSAE_GRID_CAP == EXPECT_CAP && msae_tuning::GRID_CAP == EXPECT_CAP, "cap");
static_assert(msae_tuning::grid_cap(4) == 4 && msae_tuning::grid_cap(256) == (EXPECT_CAP ? EXPECT_CAP : 256) &&
              msae_tuning::grid_cap(1 << 20) == (EXPECT_CAP ? EXPECT_CAP : 1 << 20), "grid_cap");
static_assert(PS_GEMM_TILE_ENTRY == 0 && MSAE_PERTURB_NSITES >= 20, "the sites are named with or without the switch");
int main() {
  int evaluated = 0;
  // the no-op macros drop their arguments unevaluated: neither the undeclared names nor the increments reach the compiler
  MSAE_PERTURB_AT(not_a_site + ++evaluated, ++evaluated);
  MSAE_PERTURB_AT_K(not_a_site + ++evaluated, no_such_counter);
  MSAE_PERTURB_LAUNCH(++evaluated, no_such_variable, ++evaluated);
  return evaluated;
}
"""


def _compile(tmp_path, *flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "tuning_defaults.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "tuning_defaults"
    r = subprocess.run([cxx, "-std=c++17", "-I", str(CSRC), *flags, str(src), "-o", str(exe)], capture_output=True, text=True)
    return r, exe


def test_tuning_h_defaults_are_a_noop_macro_and_no_cap(tmp_path):
    r, exe = _compile(tmp_path, "-DEXPECT_CAP=0")
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([str(exe)]).returncode == 0, "a probe macro evaluated its argument"


def test_grid_cap_switch_caps_and_rejects_what_the_tile_map_cannot_take(tmp_path):
    r, _ = _compile(tmp_path, "-DEXPECT_CAP=8", "-DMSAE_GRID_CAP=8")
    assert r.returncode == 0, r.stderr[-3000:]
    r, _ = _compile(tmp_path, "-DEXPECT_CAP=12", "-DMSAE_GRID_CAP=12")     # not a multiple of 8 (gemm_map_tile's XCD super-tile)
    assert r.returncode != 0 and "multiple of 8" in r.stderr, r.stderr[-3000:]
