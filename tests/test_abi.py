"""CPU-only: the C-ABI library loads and exports exactly what include/vlmc.h declares."""
import ctypes

import pytest

from vlmc import _lib


def test_library_exports_every_header_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _lib.header_functions()
    assert declared, "no functions parsed from include/vlmc.h"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/vlmc.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared, "vlmc/_lib.py SIGNATURES out of sync with include/vlmc.h"


def test_abi_version_and_error_string():
    lib = _lib.load()
    assert lib.vlmc_abi_version() == _lib.header_abi_version()
    assert isinstance(lib.vlmc_last_error(), bytes)


def test_workspace_query_needs_no_gpu():
    lib = _lib.load()
    assert lib.vlmc_wanda_select_workspace(_lib.SEL_ROW, 5120, 2048) == 0
    assert lib.vlmc_wanda_select_partials(_lib.SEL_ROW, 5120, 2048) == 5120
    assert lib.vlmc_wanda_select_workspace(_lib.SEL_MATRIX, 6144, 1408) >= (4096 + 2048) * 4
    assert lib.vlmc_wanda_select_workspace(7, 1, 1) == 0


def test_argument_validation_fails_loudly_without_touching_the_gpu():
    lib = _lib.load()
    rc = lib.vlmc_act_sqnorm(None, _lib.BF16, 1, 1, 8, 8, 8, None, None)
    assert rc == _lib.VLMC_EINVAL and b"null pointer" in lib.vlmc_last_error()
    with pytest.raises(_lib.VlmcError):
        _lib.check(rc)


def test_ops_refuse_cpu_tensors():
    """No CPU fallback: the product path raises instead of computing on the host."""
    import torch
    from vlmc import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.act_sqnorm(torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.wanda_select(torch.zeros(4, 8), torch.zeros(8), "row", k=2)


def test_crosscheck_list_turns_into_the_individual_switches():
    """`VLMC_CROSSCHECK=a,b` is one spelling for the cross-check routes' individual variables; explicit ones win; typos raise."""
    from vlmc import crosscheck
    env = {"VLMC_CROSSCHECK": "gemm_staged, select_multi", "VLMC_SELECT_MIXED": "1"}
    assert crosscheck.apply(env) == ["gemm_staged", "select_multi"]
    assert env["VLMC_GEMM_RING"] == "0" and env["VLMC_MATRIX_FUSED"] == "0" and env["VLMC_SELECT_MIXED"] == "1"
    env = {"VLMC_CROSSCHECK": "all"}
    assert len(crosscheck.apply(env)) == len(crosscheck.ROUTES) and env["VLMC_BATCH_REPLAY"] == "1"
    assert crosscheck.apply({}) == []
    import pytest
    with pytest.raises(ValueError):
        crosscheck.apply({"VLMC_CROSSCHECK": "gemm_stagd"})


def test_every_environment_switch_is_registered_with_its_default():
    """vlmc/config.py is the ONE list of `VLMC_*` environment variables: at most ten public ones, every other one a named cross-check
    route or an internal aid, each with a default.  A variable read anywhere in the tree -- through the readers (config.flag / integer /
    text, csrc/common.hpp's env_flag / env_int / env_text) or raw (os.environ / getenv) -- that is not listed there fails here; so does
    a raw read of a `VLMC_*` name in the package outside the readers themselves, and a C++ call site whose default is not the registry's."""
    import glob
    import os
    import re

    from vlmc import config, crosscheck
    assert len(config.PUBLIC) <= 10
    tables = (config.PUBLIC, config.CROSSCHECK, config.INTERNAL)
    assert sum(map(len, tables)) == len(config.all_names()), "a name is registered twice"
    for table in tables:
        for name, entry in table.items():
            assert isinstance(entry, tuple) and len(entry) == 2 and (entry[0] is None or isinstance(entry[0], str)) and \
                isinstance(entry[1], str) and entry[1], f"{name}: not a (default, description) pair: {entry!r}"
    routed = {k for vars_, _doc in crosscheck.ROUTES.values() for k in vars_}
    assert routed <= set(config.CROSSCHECK) | set(config.PUBLIC), sorted(routed - set(config.CROSSCHECK))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "vlm-compression_amd")
    name = r"""\(\s*["'](VLMC_[A-Z0-9_]+)["']"""
    raw = [re.compile(r"""environ(?:\.get|\.setdefault|\.pop)?""" + name), re.compile(r"""environ\[\s*["'](VLMC_[A-Z0-9_]+)"""),
           re.compile(r"""getenv""" + name), re.compile(r"""setenv""" + name)]
    readers = [re.compile(r"""config\.(?:flag|integer|text)""" + name), re.compile(r"""\benv_(?:flag|int|text)""" + name)]
    cpp_default = re.compile(r"""\benv_(flag|int)\(\s*"(VLMC_[A-Z0-9_]+)"\s*,\s*([^)]+?)\s*\)""")
    raw_ok = {os.path.join(pkg, "vlmc", "config.py"), os.path.join(pkg, "vlmc", "crosscheck.py"), os.path.join(pkg, "csrc", "common.hpp")}
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True) + glob.glob(os.path.join(pkg, "csrc", "**", "*.h*"), recursive=True) + \
        glob.glob(os.path.join(pkg, "csrc", "**", "*.cpp"), recursive=True)
    read, raw_reads, wrong_defaults = set(), [], []
    for f in files + [os.path.join(root, "bench.py")]:
        src = open(f, errors="ignore").read()
        for p in raw + readers:
            read |= set(p.findall(src))
        if f in files and f not in raw_ok:
            raw_reads += [f"{os.path.relpath(f, root)}: {n}" for p in raw for n in p.findall(src)]
        for kind, n, dflt in cpp_default.findall(src):
            want = {"true": "1", "false": "0"}.get(dflt, dflt) if kind == "flag" else dflt
            if n in config.DEFAULTS and (want.lstrip("-").isdigit() or kind == "flag") and want != config.DEFAULTS[n]:
                wrong_defaults.append(f"{os.path.relpath(f, root)}: {n} defaults to {dflt}, registered {config.DEFAULTS[n]!r}")
    unknown = sorted(read - config.all_names())
    assert not unknown, f"VLMC_* variables read but not registered in vlmc/config.py: {unknown}"
    assert not raw_reads, f"VLMC_* variables read around config.flag / integer / text or csrc/common.hpp's env_*: {raw_reads}"
    assert not wrong_defaults, wrong_defaults


def test_switch_readers_follow_one_rule(monkeypatch):
    """A flag is on unless its value is "0"; unset, every reader gives the registered default; an unregistered name raises."""
    from vlmc import config
    for value, on in (("0", False), ("1", True), ("2", True), ("", True)):
        monkeypatch.setenv("VLMC_STRICT", value)
        assert config.flag("VLMC_STRICT") is on
    monkeypatch.delenv("VLMC_STRICT")
    assert config.flag("VLMC_STRICT") is False and config.flag("VLMC_GEMM_RING") is True
    assert config.integer("VLMC_REPLAY_TOKENS") == 65536 and config.text("VLMC_LIB") is None
    monkeypatch.setenv("VLMC_REPLAY_TOKENS", "7")
    assert config.integer("VLMC_REPLAY_TOKENS") == 7 and config.text("VLMC_REPLAY_TOKENS") == "7"
    for reader in (config.flag, config.integer, config.text):
        with pytest.raises(KeyError, match="VLMC_NOT_A_SWITCH"):
            reader("VLMC_NOT_A_SWITCH")
