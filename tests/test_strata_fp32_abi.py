"""CPU-only checks of GE_ARITH_FP32's public surface: the two entry points and their argument errors, the structs that must not
have grown for it, and the `device.arith` key of the two hosts (parse, the two configuration errors, the banner line)."""
import ctypes as C
import os
import subprocess

import pytest

import geglove
from geglove import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
CFG_BYTES, INFO_BYTES = 120, 128          # sizeof(ge_glove_cfg), sizeof(ge_glove_info) before the arithmetic became a choice


def test_the_two_symbols_exist_and_refuse_a_null_handle():
    L = capi.lib()
    assert "ge_glove_set_arith" in capi.SYMBOLS and "ge_glove_get_arith" in capi.SYMBOLS
    for arith in (capi.GE_ARITH_JAVA, capi.GE_ARITH_FP32, 7):
        assert L.ge_glove_set_arith(None, arith) == capi.GE_ERR_ARG
        assert b"null" in L.ge_last_error()
    got = C.c_int32(-5)
    assert L.ge_glove_get_arith(None, C.byref(got)) == capi.GE_ERR_ARG and got.value == -5
    assert (capi.GE_ARITH_JAVA, capi.GE_ARITH_FP32) == (0, 1)


def test_cfg_and_info_did_not_grow():
    L = capi.lib()
    assert (L.ge_glove_cfg_size(), L.ge_glove_info_size()) == (CFG_BYTES, INFO_BYTES)
    assert (C.sizeof(capi.GloveCfg), C.sizeof(capi.GloveInfo)) == (CFG_BYTES, INFO_BYTES)
    assert capi.GloveCfg._fields_[-1][0] == "strata" and [f for f, _ in capi.GloveInfo._fields_[-2:]] == ["strata", "strata_path"]
    # the header itself: sizes, the two values, and the prototypes as a C compiler reads them
    src = ('#include <stdio.h>\n#include "geglove.h"\n'
           'static ge_status (*set_)(ge_glove *, int32_t) = ge_glove_set_arith;\n'
           'static ge_status (*get_)(const ge_glove *, int32_t *) = ge_glove_get_arith;\n'
           'int main(){printf("%zu %zu %d %d %d", sizeof(ge_glove_cfg), sizeof(ge_glove_info), (int)GE_ARITH_JAVA, (int)GE_ARITH_FP32, '
           'set_ != 0 && get_ != 0);return 0;}')
    exe = os.path.join(REPO, "tests", ".probe_sizes_arith")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-L", os.path.join(REPO, "graph-embeddings_amd", "lib"),
                    "-lgeglove", "-Wl,-rpath," + os.path.join(REPO, "graph-embeddings_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                   input=src.encode(), check=True)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    finally:
        os.remove(exe)
    assert got == [CFG_BYTES, INFO_BYTES, 0, 1, 1]


# ---------------------------------------------------------------- the YAML key in both hosts
YAML = ("graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
        "device:\n  mode: %s\n  shuffle: device\n%s")


@pytest.fixture(scope="module")
def host():
    capi._share_hip_runtime_with_torch()
    L = C.CDLL(os.environ.get("GE_HOST_LIB") or os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    L.geh_config_summary.restype = C.c_char_p
    return L


def _summary(host, tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return host.geh_config_summary(str(p).encode(), 1).decode()


def test_the_cpp_host_parses_the_key_and_prints_the_banner_line_only_with_fp32(host, tmp_path):
    plain = _summary(host, tmp_path, "plain.yml", YAML % ("stratified", "  strata: 4\n")).splitlines()
    java = _summary(host, tmp_path, "java.yml", YAML % ("stratified", "  strata: 4\n  arith: java\n")).splitlines()
    fp32 = _summary(host, tmp_path, "fp32.yml", YAML % ("stratified", "  strata: 4\n  arith: fp32\n")).splitlines()
    assert plain[0] == java[0] == fp32[0] == "OK"
    assert plain == java and "# Stratified trainer: 4 strata" in plain and not any("arithmetic" in l for l in plain)
    # one more line, right behind the trainer's, and every other line as it was
    at = fp32.index("# Stratified trainer: 4 strata")
    assert fp32[at + 1] == "# Stratified arithmetic: fp32"
    assert fp32[:at + 1] + fp32[at + 2:] == plain
    auto = _summary(host, tmp_path, "auto.yml", YAML % ("stratified", "  arith: fp32\n")).splitlines()
    assert "# Stratified trainer: strata chosen from the matrix" in auto and "# Stratified arithmetic: fp32" in auto
    tiny = host.geh_config_summary(os.path.join(GOLD, "tiny.config.yml").encode(), 1).decode()
    assert tiny.startswith("OK") and "Stratified" not in tiny


def test_the_cpp_host_refuses_fp32_outside_the_stratified_mode_and_unknown_words(host, tmp_path):
    for mode in ("hogwild", "deterministic"):
        out = _summary(host, tmp_path, mode + ".yml", YAML % (mode, "  arith: fp32\n"))
        assert out == "ERR\nInvalid configuration: device.arith: fp32 needs device.mode: stratified", out
        assert _summary(host, tmp_path, mode + "_java.yml", YAML % (mode, "  arith: java\n")).startswith("OK")
    for word in ("fp64", "FP32", "fast", ""):
        out = _summary(host, tmp_path, "word.yml", YAML % ("stratified", "  arith: %s\n" % (word or '""')))
        assert out == "ERR\nInvalid configuration: Invalid device.arith, choose one of: java, fp32", (word, out)


def _config(**device):
    return geglove.Configuration(dict(graph="g", method="glove", dim=4, threads=1, bca={"alpha": .1, "epsilon": 1e-3},
                                      opt={"maxiter": 1}, output={"uri": []}, device=device))


def test_the_python_host_validates_the_key_before_any_device_work(tmp_path):
    p = tmp_path / "fp32.yml"
    p.write_text(YAML % ("stratified", "  strata: 4\n  arith: fp32\n"))
    py = geglove.Configuration.load(str(p))
    assert py.device["arith"] == "fp32" and py.device["mode"] == "stratified"
    geglove.Configuration.check(py)
    assert geglove.host._ARITH == {"java": capi.GE_ARITH_JAVA, "fp32": capi.GE_ARITH_FP32}
    m = geglove.CooMatrix(3, [0, 1], [1, 2], [0.1, 0.1], 0.2)
    no_device = 1 << 20                       # a handle that got past the configuration fails at selecting this device
    for dev, what in ((dict(mode="hogwild", arith="fp32"), "device.arith: fp32 needs device.mode: stratified"),
                      (dict(mode="deterministic", shuffle="none", arith="fp32"), "device.arith: fp32 needs device.mode: stratified"),
                      (dict(arith="fp32"), "device.arith: fp32 needs device.mode: stratified"),
                      (dict(mode="stratified", arith="double"), "Invalid device.arith, choose one of: java, fp32")):
        cfg = _config(id=no_device, **dev)
        with pytest.raises(geglove.host.InvalidConfigurationException) as e:
            geglove.Configuration.check(cfg)
        assert str(e.value) == "Invalid configuration: " + what
        with pytest.raises(geglove.host.InvalidConfigurationException) as e:
            geglove.Adagrad(m, cfg, cfg.costFunction())
        assert str(e.value) == "Invalid configuration: " + what
    for dev in (dict(mode="stratified", arith="fp32"), dict(mode="stratified", arith="java"), dict(mode="hogwild", arith="java")):
        cfg = _config(id=no_device, **dev)
        geglove.Configuration.check(cfg)
        with pytest.raises(geglove.GeError):   # the configuration is fine: only the device is missing
            geglove.Adagrad(m, cfg, cfg.costFunction())
