"""The native library's DVSR_* environment switches: one table (csrc/switches.h), read at one site (csrc/switches.hip), and every
other list of them -- the engine's plan-cache key, its warn-on-change list, INTEGRATION.md -- taken from or held against that table
through the host queries dvsr_switch_count / _info / _parse / _value.  No device: the queries launch nothing."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import warnings

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dynavsr_amd", "csrc")
BUILD, PROCESS, CALL, DEBUG = 0, 1, 2, 3   # DVSR_SW_* of include/dynavsr_hip.h
# the 30 switches and when the library reads each: what the code did before the table existed, stated here, not taken from the library
SCOPES = {
    BUILD: "CONV_WINO CONV_WINO3 CONV_WINO5 CONV_V1 EST_SPLIT EST_SPLIT2 FUSE_ACT_BWD BWD_STREAMS PCD_HOIST",
    PROCESS: "CONV_LAST_MFMA SPLIT_TH8_FROM WGRAD_SPLIT3 WGRAD_WIDE WGRAD_S3V WGRAD_S3W WGRAD_S3_KYS_BELOW WGRAD_S3_WGS DCN_FWD DCN_BWD "
             "EST_FUSE_PAD FUSE_RES_BWD BWD_FORK_EVERY BWD_PROBE TSA_DUAL TSA_V UP2",
    CALL: "DEGRADE_GENERIC",
    DEBUG: "CONV_LDS CONV_ABLATE WGRAD_NOFLUSH",
}
SCOPES = {scope: {"DVSR_" + n for n in names.split()} for scope, names in SCOPES.items()}
# parser classes: {switch: value when unset}, and the mapping of every string (None: unset) the sites made before the table
ATOI = {"CONV_WINO": 1, "CONV_WINO3": 1, "CONV_WINO5": 1, "EST_SPLIT": 1, "EST_SPLIT2": 1, "SPLIT_TH8_FROM": 200, "WGRAD_S3_KYS_BELOW": 4000,
        "WGRAD_S3_WGS": 0, "BWD_FORK_EVERY": 0, "TSA_V": 2, "CONV_ABLATE": 0, "WGRAD_NOFLUSH": 0, "CONV_LDS": 0}
PARSERS = [
    ("BWD_PROBE WGRAD_WIDE WGRAD_S3V WGRAD_S3W WGRAD_SPLIT3 TSA_DUAL FUSE_RES_BWD FUSE_ACT_BWD BWD_STREAMS EST_FUSE_PAD PCD_HOIST".split(),
     {None: 1, "": 1, "0": 0, "0x": 0, "1": 1, "x": 1}),                                                  # on unless 0...
    (["CONV_V1", "CONV_LAST_MFMA"], {None: 0, "": 0, "0": 0, "1": 1, "1x": 1, "2": 0}),                  # on iff 1...
    (list(ATOI), {None: "default", "": 0, "x": 0, "3": 3, "-1": -1}),                                   # atoi
    (["DEGRADE_GENERIC"], {None: 0, "": 1, "0": 1, "1": 1}),                                             # on iff set
    (["UP2"], {None: 0, "": 0, "4": 1, "4x": 1, "2": 0, "x": 0}),
    (["DCN_FWD"], {None: 3, "": 3, "s": 3, "split": 3, "r": 2, "reg": 2, "dma": 0, "lds": 0, "x": 0, "0": 0}),
    (["DCN_BWD"], {None: 0, "": 0, "u": 1, "unfused": 1, "f": 2, "fp32": 2, "x": 0, "0": 0, "1": 0}),
]


@pytest.fixture(scope="module")
def table():
    from dynavsr_amd import _lib as L
    return L.switches()


def _index(table, name):
    return [r[0] for r in table].index(name)


def _parse(table, name, text):
    from dynavsr_amd import _lib as L
    v = ctypes.c_int(-12345)
    L.check(L.lib().dvsr_switch_parse(_index(table, name), None if text is None else text.encode(), ctypes.byref(v)), "dvsr_switch_parse")
    return v.value


def _sources():
    return [f for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))]


def test_one_reading_site():
    """No getenv("DVSR_...") in csrc/ outside switches.hip (the guard against a new stray site); every Sw:: name a site uses is a
    row of the table, and every row has a site."""
    stray = [os.path.basename(f) for f in _sources()
             if os.path.basename(f) != "switches.hip" and re.search(r'getenv\s*\(\s*"DVSR_', open(f).read())]
    assert not stray, stray
    from dynavsr_amd import _lib as L
    used = set()
    for f in _sources():
        used |= set(re.findall(r"\bSw::([A-Z0-9_]+)", open(f).read()))
    used -= {"COUNT"}
    assert {"DVSR_" + n for n in used} == {r[0] for r in L.switches()}, used


def test_table_holds_the_thirty_switches_with_their_scopes(table):
    assert len(table) == 30 and len({r[0] for r in table}) == 30
    for scope, names in SCOPES.items():
        assert {r[0] for r in table if r[1] == scope} == names, scope
    for name, _scope, dflt, doc in table:
        assert doc.strip() and _parse(table, name, None) == dflt, name


def test_engine_lists_are_the_tables(table, monkeypatch):
    """The plan-cache key is the BUILD set, the warn-on-change list the PROCESS set; a PROCESS switch changed between two plan builds
    warns (the native side keeps what it read first), DVSR_DEGRADE_GENERIC -- read on every call -- does not."""
    from dynavsr_amd import _lib as L, engine
    assert set(L.switch_names(L.SW_BUILD)) == SCOPES[BUILD] and set(L.switch_names(L.SW_PROCESS)) == SCOPES[PROCESS]
    for k in SCOPES[BUILD]:
        monkeypatch.delenv(k, raising=False)
    base = engine._env_key()
    assert len(base) == len(SCOPES[BUILD])
    for k in SCOPES[BUILD]:
        monkeypatch.setenv(k, "7")
        assert engine._env_key() != base, k
        monkeypatch.delenv(k)
    monkeypatch.setattr(engine, "_process_env_seen", None)
    monkeypatch.delenv("DVSR_DCN_FWD", raising=False)
    monkeypatch.delenv("DVSR_DEGRADE_GENERIC", raising=False)
    engine._check_process_env()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        engine._check_process_env()
        assert not w
        monkeypatch.setenv("DVSR_DEGRADE_GENERIC", "1")
        monkeypatch.setenv("DVSR_CONV_LDS", "4096")
        engine._check_process_env()
        assert not w
        monkeypatch.setenv("DVSR_DCN_FWD", "dma")
        engine._check_process_env()
        assert len(w) == 1 and "DVSR_DCN_FWD" in str(w[0].message)


@pytest.mark.parametrize("row", range(len(PARSERS)))
def test_parser_rows(table, row):
    names, mapping = PARSERS[row]
    for n in names:
        for text, want in mapping.items():
            want = ATOI[n] if want == "default" else want
            assert _parse(table, "DVSR_" + n, text) == want, (n, text)


def test_every_switch_is_in_one_parser_class(table):
    assert sorted("DVSR_" + n for names, _m in PARSERS for n in names) == sorted(r[0] for r in table)


def test_a_build_switch_follows_the_environment(table, monkeypatch):
    from dynavsr_amd import _lib as L
    monkeypatch.delenv("DVSR_CONV_WINO5", raising=False)
    assert L.switch_value("DVSR_CONV_WINO5") == 1
    monkeypatch.setenv("DVSR_CONV_WINO5", "3")
    assert L.switch_value("DVSR_CONV_WINO5") == 3
    monkeypatch.setenv("DVSR_CONV_WINO5", "0")
    assert L.switch_value("DVSR_CONV_WINO5") == 0
    monkeypatch.setenv("DVSR_CONV_V1", "yes")     # neither 0... nor 1...: the engine never took this for v1
    assert L.switch_value("DVSR_CONV_V1") == 0
    monkeypatch.setenv("DVSR_CONV_V1", "1")
    assert L.switch_value("DVSR_CONV_V1") == 1


_CHILD = r"""
import ctypes, os, sys
lib = ctypes.CDLL(sys.argv[1])
def value(i):
    v = ctypes.c_int(-12345)
    assert lib.dvsr_switch_value(i, ctypes.byref(v)) == 0
    return v.value
tsa_v, up2, generic = (int(a) for a in sys.argv[2:5])
os.environ["DVSR_TSA_V"] = "4"
os.environ.pop("DVSR_UP2", None)
os.environ.pop("DVSR_DEGRADE_GENERIC", None)
out = [value(tsa_v), value(generic)]
os.environ["DVSR_TSA_V"] = "1"          # kept from its first read
os.environ["DVSR_UP2"] = "4"            # not read yet: its own first use comes now
os.environ["DVSR_DEGRADE_GENERIC"] = "0"
out += [value(tsa_v), value(up2), value(generic)]
os.environ.pop("DVSR_UP2")
out += [value(up2)]
print(*out)
"""


def test_a_process_switch_keeps_its_first_read(table):
    """In a child that loads only the library (the suite's own process keeps its first reads for the tests that need them): a PROCESS
    switch is read at ITS first use -- not at the first use of another -- and kept; a CALL switch follows the environment."""
    from dynavsr_amd import _lib as L
    r = subprocess.run([sys.executable, "-c", _CHILD, os.environ.get("DVSR_HIP_LIB", L.SO_PATH)] +
                       [str(_index(table, n)) for n in ("DVSR_TSA_V", "DVSR_UP2", "DVSR_DEGRADE_GENERIC")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["4", "0", "4", "1", "1", "1"], r.stdout


def test_integration_md_lists_the_table(table):
    """Every switch is in INTEGRATION.md's section on environment variables, and every DVSR_* name there is a switch, one of the
    Python-side product settings, or a constant of the C header."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("### Environment variables"):]
    section = section[:section.index("\n## ")]
    named = set(re.findall(r"DVSR_[A-Z0-9_]+", section))
    names = {r[0] for r in table}
    assert not names - named, names - named
    header = set(re.findall(r"#define (DVSR_[A-Z0-9_]+)", open(os.path.join(ROOT, "include", "dynavsr_hip.h")).read()))
    other = named - names - {"DVSR_ASYNC_PNG", "DVSR_HIP_LIB"} - header
    assert not other, other
