"""CPU tier: the surface of the chain diagnostics (include/lmc_abi.h "Chain diagnostics": lmc_chain_rows, lmc_chain_trace_begin / _read / _end,
lmc_step_table, lmc_set_option "step_table"; the Python bindings; dpt_amd's flags) and the reader of dpt_amd's trace files.  The GPU tier is
tests/test_gpu_chain_diag.py."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc

CALLS = ("lmc_chain_rows", "lmc_chain_trace_begin", "lmc_chain_trace_read", "lmc_chain_trace_end", "lmc_step_table")
CSRC = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc")


def _read(*parts):
    return open(os.path.join(gc.ROOT, *parts)).read()


def test_the_five_calls_are_declared_exported_and_bound():
    hdr = _read("include", "lmc_abi.h")
    assert re.search(r"#define\s+LMC_ROW_WORDS\s+48\b", hdr)
    assert re.search(r"int\s+lmc_chain_rows\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+which\s*,\s*const\s+int\s*\*\s*chain_ids\s*,\s*int\s+n\s*,\s*float\s*\*\s*out\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_chain_trace_begin\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const\s+int\s*\*\s*chain_ids\s*,\s*int\s+n\s*,\s*int\s+capacity_steps\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_chain_trace_read\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*float\s*\*\s*rows\s*,\s*int\s+cap_steps\s*,\s*long long\s*\*\s*first_step\s*,\s*int\s*\*\s*n_steps\s*,"
                     r"\s*long long\s*\*\s*dropped\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_chain_trace_end\s*\(\s*lmc_ctx\s*\*\s*ctx\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_step_table\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*out\s*,\s*int\s+clear\s*\)\s*;", hdr)
    assert '"step_table"' in hdr and "Chain diagnostics" in hdr and "resident" in hdr.split("Chain diagnostics", 1)[1]
    p = gc.pkg()
    L = ctypes.CDLL(p.LIB_PATH)
    for fn in CALLS:
        assert hasattr(L, fn), fn
        assert getattr(p.lib(), fn).argtypes is not None, fn
    for m in ("chain_rows", "trace_chains", "trace_read", "trace_end", "step_table"):
        assert callable(getattr(p.Renderer, m, None)), m
    assert callable(p.trace_file_read) and p.ROW_WORDS == 48


def test_the_units_are_where_the_documents_say():
    mk = _read("langevin-mcmc_amd", "csrc", "Makefile")
    assert re.search(r"^HOST_HIP\s*:=.*\bchaindiag\b", mk, re.M) and re.search(r"^DEVICE_TUS\s*:=.*\bchaindiag\b", mk, re.M)
    # only the device unit that shares a host unit's name gets another object name: the other objects keep theirs (tests/test_host.py links four of them)
    assert "$(OBJ)/%_dev.o: $(SRC)/device/%.hip" in mk and re.search(r"^\$\(foreach t,\$\(HOST_CXX\),\$\(OBJ\)/\$\(t\)\.o\)", mk, re.M)
    host, dev, core = _read(CSRC, "host", "chaindiag.cpp"), _read(CSRC, "device", "chaindiag.hip"), _read(CSRC, "host", "context.cpp")
    assert "__global__" not in host and "hipLaunchKernelGGL" not in host  # host code only, as tests/test_host_units.py asks of the host units
    for fn in CALLS:
        assert re.search(r"^int " + fn + r"\(", host, re.M), fn
        assert fn + "(" not in core, fn
    for k in ("k_chain_rows", "k_step_table", "k_latch_kind"):
        assert re.search(r"__global__ void (__launch_bounds__\(\d+\) )?" + k + r"\(", dev), k
    kh = _read(CSRC, "device", "kernels.h")
    for fn in ("LaunchChainRows", "LaunchStepTable", "LaunchLatchKind"):
        assert fn + "(" in kh and fn + "(" in dev, fn
    # the hooks of the step path: calls into lmc_host::, each behind the one pointer
    for hook in ("DiagStepBegin(c, cur)", "DiagStepEnd(c)", "DiagChainsReset(c)", "DiagNeedsLockStep(c)"):
        assert ("if (c->diag) " + hook) in core or ("if (c->diag && " + hook) in core, hook
    assert "DiagFree(ctx)" in core
    for doc, what in (("INTEGRATION.md", "## Chain diagnostics"), ("DESIGN.md", "chaindiag"), ("README.md", "lmc_chain_rows")):
        assert what in _read(doc), doc


def test_the_option_is_in_both_option_tables():
    core = _read(CSRC, "host", "context.cpp")
    setter, getter = core.split("int lmc_set_option(")[1].split("int lmc_get_option(")[0], core.split("int lmc_get_option(")[1].split("lmc_output_name")[0]
    assert 'n == "step_table"' in setter and 'n == "step_table"' in getter


def test_dpt_amd_help_names_the_flags():
    exe = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")
    gc.pkg()  # the package's import does not build; the library and the tool come from build()
    assert os.path.exists(exe), "langevin-mcmc_amd/dpt_amd is missing (python __graft_entry__.py)"
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    for flag in ("--trace-chains", "--trace-file", "--trace-steps", "--step-table"):
        assert flag in r.stdout, flag
    src = _read("tools", "dpt_amd.cpp")
    for s in ("lmc_chain_trace_begin", "lmc_chain_trace_read", "lmc_step_table", '"step_table"', "LMCTRACE"):
        assert s in src, s


def _trace_bytes(ids, first, rows, version=1, words=48):
    steps, n = rows.shape[:2]
    b = b"LMCTRACE" + struct.pack("<IIII", version, words, n, steps) + struct.pack("<q", first)
    for i in ids:
        b += struct.pack("<i", int(i))
    for v in rows.reshape(-1):
        b += struct.pack("<f", float(v))
    return b


def test_trace_file_read(tmp_path):
    p = gc.pkg()
    rng = np.random.default_rng(1)
    ids = np.array([5, 0, 4096, 77], np.int32)
    rows = rng.standard_normal((3, 4, 48)).astype(np.float32)
    rows[1, 2, 40] = -1.0
    path = str(tmp_path / "t.lmctrace")
    open(path, "wb").write(_trace_bytes(ids, 1234567890123, rows))
    t = p.trace_file_read(path)
    assert np.array_equal(t["ids"], ids) and t["ids"].dtype == np.int32
    assert t["first_step"] == 1234567890123
    assert t["rows"].shape == (3, 4, 48) and t["rows"].dtype == np.float32 and np.array_equal(t["rows"].view(np.uint32), rows.view(np.uint32))
    empty = str(tmp_path / "e.lmctrace")
    open(empty, "wb").write(_trace_bytes(ids, 1, rows[:0]))
    assert p.trace_file_read(empty)["rows"].shape == (0, 4, 48)
    for name, data in (("magic", b"LMCTRACF" + _trace_bytes(ids, 1, rows)[8:]), ("version", _trace_bytes(ids, 1, rows, version=2)), ("short", _trace_bytes(ids, 1, rows)[:-4]),
                       ("long", _trace_bytes(ids, 1, rows) + b"\0")):
        bad = str(tmp_path / (name + ".lmctrace"))
        open(bad, "wb").write(data)
        with pytest.raises(ValueError):
            p.trace_file_read(bad)
