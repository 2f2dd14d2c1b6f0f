"""bin/lw_spectra and bin/sw_spectra with scenarios=TABLE as a user would run them: every OUTPUT of a table run against the file
the same tool writes when run alone with `output=OUTPUT` and the line's scalings as `scaling=` / `conc=` - every dimension,
variable and attribute, value for value, the attributes `history`, `config` and `scenario` apart.  The comparison is exact:
the merged matrix of a scenario has the bits of the gas-by-gas merge (tests/test_merge_scenario_gpu.py) and the same kernels run
on it.  Also: one read of every input per column, the host mirror, the refusals with and without a device, and the chain
ckdmip_lw --scenarios + lw_spectra scenarios= -> optimize_lut against the same chain made of single runs."""
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn
from test_cli_optimize_gpoints_gpu import KEYS, WEIGHT, chain  # noqa: F401  (the fixture of the optimiser's tool test)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, NLAY, NWAV, NG = 2, 7, 1531, 5
GASES = {"h2o": (41, 3.0, 5e-3), "co2": (43, 0.8, 4e-4), "ch4": (47, 0.3, 1.8e-6)}
INPUT = "input=h2o.nc co2.nc ch4.nc"
MU0 = "cos_solar_zenith_angle=0.3 0.8"
PARAMETER_ERROR = 147
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
# NAME, and per gas file (scaling, conc) as the single run takes them; -1: the key's "not given"
LINES = (("base", ((-1, -1), (-1, -1), (-1, -1))),
         ("half", ((0.5, -1), (-1, -1), (2, -1))),
         ("mixed", ((-1, 3e-3), (1.5, -1), (-1, -1))),
         ("again", ((0.5, -1), (-1, -1), (2, -1))))


def _tool(name, *args, cwd=None, env=None):
    exe = os.path.join(ROOT, "bin", name)
    if not os.path.exists(exe):                      # a fresh checkout: build the library and the tools first
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return subprocess.run([exe, *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **env) if env else None)


def _ok(r):
    assert r.returncode == 0, r.stderr + r.stdout
    return r


def _nc(path):
    return netcdf_file(str(path), "r", mmap=False)


def _spec(scaling, conc):
    return f"scale={scaling}" if scaling >= 0 else f"conc={conc}" if conc >= 0 else "asis"


def _table(path, lines, suffix, extension="nc"):
    """the table of `lines` with outputs t_<name>_<suffix>; comments and blank lines as the grammar allows them"""
    text = "# NAME OUTPUT one spec per input file\n\n"
    for name, specs in lines:
        text += f"{name}  t_{name}_{suffix}.{extension}  " + " ".join(_spec(s, c) for s, c in specs) + "   # a comment\n"
    path.write_text(text)


def _single_keys(specs):
    return ("scaling=" + " ".join(str(s) for s, _ in specs), "conc=" + " ".join(str(c) for _, c in specs))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three gas files of NCOL columns (FLOAT optical depths, mole fractions, a reference surface mole fraction), g points with
    some wavenumbers unassigned, an ssi file and a spectrum that scatters"""
    d = tmp_path_factory.mktemp("spectra_scenarios")
    p = syn.pressure_grid(NLAY)
    t = np.stack([syn.temperature_profile(p) + 3.0 * c for c in range(NCOL)])
    wn, dwn = syn.wavenumber_grid(NWAV, 250.0, 3000.0)

    def spectrum(name, od, vmr=None, molecule=None):
        w = netcdf_file(str(d / name), "w", version=2)
        for dim, n in (("column", NCOL), ("half_level", NLAY + 1), ("level", NLAY), ("wavenumber", NWAV)):
            w.createDimension(dim, n)
        w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p, (NCOL, 1))
        w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = t
        w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
        if vmr is not None:
            w.createVariable("mole_fraction_fl", "d", ("column", "level"))[:] = vmr * (1.0 + 0.1 * np.arange(NLAY))[None, :] * np.ones((NCOL, 1))
            w.createVariable("reference_surface_mole_fraction", "d", ())[...] = vmr
        w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od
        w.constituent_id = molecule or name[:-3]
        w.close()
    for g, (seed, scale, vmr) in GASES.items():
        od0 = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=24, column_scale=scale, dtype="float32", lo=250.0, hi=3000.0)
        spectrum(f"{g}.nc", np.stack([(od0 * np.float32(1.0 + 0.25 * c)).astype(np.float32) for c in range(NCOL)]), vmr)
    ray = np.diff(p)[:, None] / p[-1] * (0.4 * (wn / 3000.0) ** 4)[None, :]
    spectrum("rayleigh.nc", np.stack([(ray * (1.0 + 0.1 * c)).astype(np.float32) for c in range(NCOL)]), molecule="rayleigh")
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", NWAV)
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.close()
    rng = np.random.default_rng(11)
    g_point = rng.integers(0, NG, size=NWAV).astype(np.int32)
    g_point[rng.random(NWAV) < 0.05] = -1
    w = netcdf_file(str(d / "gpoints.nc"), "w", version=2)
    w.createDimension("wavenumber", NWAV)
    w.createVariable("g_point", "i", ("wavenumber",))[:] = g_point
    w.close()
    return dict(d=d, ssi=ssi, g_point=g_point)


def _assert_same_file(table_file, single_file, scenario):
    a, b = _nc(table_file), _nc(single_file)
    try:
        assert a.dimensions == b.dimensions and list(a.variables) == list(b.variables)
        for name, v in a.variables.items():
            w = b.variables[name]
            assert v.dimensions == w.dimensions and v.data.dtype == w.data.dtype and v._attributes == w._attributes, name
            assert np.array_equal(v[...], w[...]), (scenario, name)
        apart = {"history", "config", "scenario"}
        assert {k: v for k, v in a._attributes.items() if k not in apart} == {k: v for k, v in b._attributes.items() if k not in apart}
        assert set(a._attributes) - set(b._attributes) == {"scenario"} and a.scenario == scenario.encode()
        assert b"scenarios=" in a.config and b"scenarios" in a.history
    finally:
        a.close(); b.close()


def _table_against_singles(d, tool, keys, suffix, lines=LINES, input_key=INPUT):
    """the table run, then every line alone; -> the table run's log"""
    _table(d / f"table_{suffix}.txt", lines, suffix)
    r = _ok(_tool(tool, input_key, *keys, f"scenarios=table_{suffix}.txt", cwd=d))
    for name, specs in lines:
        _ok(_tool(tool, input_key, *keys, *_single_keys(specs), f"output=s_{name}_{suffix}.nc", cwd=d))
        _assert_same_file(d / f"t_{name}_{suffix}.nc", d / f"s_{name}_{suffix}.nc", name)
    return r.stdout


def _assert_repeat_equals(d, suffix):
    a, b = _nc(d / f"t_half_{suffix}.nc"), _nc(d / f"t_again_{suffix}.nc")
    for name in a.variables:
        assert np.array_equal(a.variables[name][...], b.variables[name][...]), name
    assert not np.array_equal(a.variables["optical_depth"][...], _nc(d / f"t_base_{suffix}.nc").variables["optical_depth"][...])


@pytest.mark.parametrize("nangle", [0, 2])
def test_lw_spectra_per_g_point(files, nangle):
    d = files["d"]
    log = _table_against_singles(d, "lw_spectra", ("gpoints=gpoints.nc", *([f"nangle={nangle}"] if nangle else [])), f"lw{nangle}")
    _assert_repeat_equals(d, f"lw{nangle}")
    f = _nc(d / f"t_mixed_lw{nangle}.nc")
    assert f.dimensions["column"] is None and f.variables["optical_depth"].shape == (NCOL, NLAY, NG)
    assert (getattr(f, "nangle", 0) or 0) == nangle
    # one read of every input per column, whatever the number of lines
    reading = [line for line in log.splitlines() if line.strip().startswith("Reading")]
    for g in GASES:
        assert sum(f"{g}.nc" in line for line in reading) == NCOL, log
    assert sum("Scenario " in line for line in log.splitlines()) == NCOL * len(LINES)


@pytest.mark.parametrize("rayleigh", [False, True], ids=["absorbing", "rayleigh"])
def test_sw_spectra_per_g_point(files, rayleigh):
    d = files["d"]
    suffix = "swr" if rayleigh else "sw"
    log = _table_against_singles(d, "sw_spectra", ("gpoints=gpoints.nc", "ssi=ssi.nc", MU0, *(["rayleigh=rayleigh.nc"] if rayleigh else [])), suffix)
    _assert_repeat_equals(d, suffix)
    f = _nc(d / f"t_half_{suffix}.nc")
    assert f.variables["spectral_flux_up_sw"].shape == (NCOL, 2, NLAY + 1, NG)
    assert ("rayleigh_optical_depth" in f.variables) == rayleigh and hasattr(f, "rayleigh_scattering") == rayleigh
    if rayleigh:                                     # the spectrum that scatters is never scaled
        g = _nc(d / "t_base_swr.nc")
        assert np.array_equal(f.variables["rayleigh_optical_depth"][...], g.variables["rayleigh_optical_depth"][...])
        reading = [line for line in log.splitlines() if line.strip().startswith("Reading")]
        assert sum("h2o.nc" in line for line in reading) == NCOL


def test_lw_spectra_per_wavenumber(files):
    d = files["d"]
    _table_against_singles(d, "lw_spectra", (), "lwwn", lines=LINES[:3])
    f = _nc(d / "t_half_lwwn.nc")
    assert f.variables["optical_depth"].shape == (NCOL, NLAY, NWAV) and "wavenumber" in f.variables


def test_netcdf4_outputs(files):
    from ecckd_amd import ncio
    d = files["d"]
    lines = LINES[1:3]
    _table(d / "table_h5.txt", lines, "h5", extension="h5")
    _ok(_tool("lw_spectra", INPUT, "gpoints=gpoints.nc", "scenarios=table_h5.txt", cwd=d))
    names = ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw", "spectral_flux_up_lw")
    for name, specs in lines:
        h5 = d / f"t_{name}_h5.h5"
        assert h5.read_bytes()[:8] == b"\x89HDF\r\n\x1a\n"
        _ok(_tool("lw_spectra", INPUT, "gpoints=gpoints.nc", *_single_keys(specs), f"output=s_{name}_h5.h5", cwd=d))
        with ncio.NcFile(h5) as a, ncio.NcFile(d / f"s_{name}_h5.h5") as b:
            assert a.dim("column") == NCOL == b.dim("column") and a.dim("g_point") == NG
            for v in names:
                assert a.var_info(v) == b.var_info(v), v
                assert np.array_equal(a.read(v), b.read(v)), (name, v)
            assert a.att_text("scenario") == name and a.att_text("molecules") == b.att_text("molecules")


def test_single_input_unscaled_and_scaled(files):
    """one input: the unscaled line takes the matrix as stored (FLOAT), the scaled line beside it the merged DOUBLE one"""
    d = files["d"]
    lines = (("asis", ((-1, -1),)), ("double", ((2, -1),)))
    _table_against_singles(d, "lw_spectra", ("gpoints=gpoints.nc",), "one", lines=lines, input_key="input=h2o.nc")
    _table_against_singles(d, "lw_spectra", ("iprofile=1",), "onewn", lines=lines, input_key="input=h2o.nc")
    a, b = _nc(d / "t_asis_onewn.nc"), _nc(d / "t_double_onewn.nc")
    assert a.variables["optical_depth"].shape == (1, NLAY, NWAV)
    assert np.array_equal(b.variables["optical_depth"][...], (2.0 * a.variables["optical_depth"][...].astype(np.float64)).astype(np.float32))


def test_host_mirror(ctx, files):
    """pipeline.lw_spectra / sw_spectra (scenarios=) return, per scenario, the arrays of the tool's file to the FLOAT"""
    from ecckd_amd import pipeline
    d = files["d"]
    inputs = [d / f"{g}.nc" for g in GASES]
    as_list = lambda specs, i: None if all(s[i] < 0 for s in specs) else [s[i] for s in specs]
    scenarios = [dict(name=name, output=d / f"py_{name}.nc", scaling=as_list(specs, 0), conc=as_list(specs, 1)) for name, specs in LINES[:3]]
    _table(d / "table_pylw.txt", LINES[:3], "pylw")
    _ok(_tool("lw_spectra", INPUT, "gpoints=gpoints.nc", "nangle=2", "scenarios=table_pylw.txt", cwd=d))
    got = pipeline.lw_spectra(ctx, inputs, g_point=files["g_point"], nangle=2, scenarios=scenarios)
    assert isinstance(got, list) and [m["scenario"] for m in got] == [name for name, _ in LINES[:3]]
    for (name, _), m in zip(LINES[:3], got):
        f, g = _nc(d / f"t_{name}_pylw.nc"), _nc(d / f"py_{name}.nc")
        for v in f.variables:
            assert np.array_equal(np.asarray(m[v]).astype(np.float32), f.variables[v][...]), (name, v)
            assert np.array_equal(g.variables[v][...], f.variables[v][...]), (name, v)
        assert g.scenario == name.encode() and g.dimensions == f.dimensions
    _table(d / "table_pysw.txt", LINES[:3], "pysw")
    _ok(_tool("sw_spectra", INPUT, "gpoints=gpoints.nc", "ssi=ssi.nc", MU0, "rayleigh=rayleigh.nc", "scenarios=table_pysw.txt", cwd=d))
    for s in scenarios:
        s["output"] = None
    got = pipeline.sw_spectra(ctx, inputs, files["ssi"], g_point=files["g_point"], cos_sza=(0.3, 0.8), rayleigh=d / "rayleigh.nc",
                              scenarios=scenarios)
    for (name, _), m in zip(LINES[:3], got):
        f = _nc(d / f"t_{name}_pysw.nc")
        for v in f.variables:
            assert np.array_equal(np.asarray(m[v]).astype(np.float32), f.variables[v][...]), (name, v)
    # without the argument the functions return what they returned: one dict
    assert isinstance(pipeline.lw_spectra(ctx, inputs[:1], g_point=files["g_point"], iprofile=0), dict)


GP = ("lw_spectra", (INPUT, "gpoints=gpoints.nc"))
SW = ("sw_spectra", (INPUT, "gpoints=gpoints.nc", "ssi=ssi.nc", "rayleigh=rayleigh.nc"))
GOOD = "a refused_a.nc asis asis asis\n"
REFUSALS = {
    "table_missing": (GP, None, "Cannot open scenario table"),
    "table_empty": (GP, "# nothing\n\n", "is empty"),
    "too_few_specs": (GP, GOOD + "b refused_b.nc asis scale=2\n", "table.txt:2: 2 scaling spec(s) for 3 spectrum file(s)"),
    "too_many_specs": (GP, "b refused_b.nc asis asis asis asis\n", "table.txt:1: 4 scaling spec(s) for 3 spectrum file(s)"),
    "unknown_spec": (GP, "b refused_b.nc asis double=2 asis\n", 'unknown scaling spec "double=2"'),
    "no_number": (GP, "b refused_b.nc asis scale= asis\n", "no number after '='"),
    "const": (GP, GOOD + "b refused_b.nc asis const=1e-4 asis\n", "const=C is not a scaling of lw_spectra"),
    "duplicate_output": (GP, GOOD + "b refused_a.nc scale=2 asis asis\n", 'duplicate output file "refused_a.nc"'),
    "output_is_an_input": (GP, GOOD + "b ./co2.nc scale=2 asis asis\n", "is the input file of this run"),
    "output_is_the_gpoints": (GP, GOOD + "b gpoints.nc scale=2 asis asis\n", "is the gpoints file of this run"),
    "output_is_the_ssi": (SW, GOOD + "b ssi.nc scale=2 asis asis\n", "is the ssi file of this run"),
    "output_is_the_rayleigh": (SW, GOOD + "b rayleigh.nc scale=2 asis asis\n", "is the rayleigh file of this run"),
    "output_beside": ((GP[0], GP[1] + ("output=refused_b.nc",)), GOOD, '"output" cannot be combined with "scenarios"'),
    "scaling_beside": ((GP[0], GP[1] + ("scaling=1 1 1",)), GOOD, '"scaling" cannot be combined with "scenarios"'),
    "conc_beside": ((GP[0], GP[1] + ("conc=1e-3 -1 -1",)), GOOD, '"conc" cannot be combined with "scenarios"'),
    "conc_input_beside": ((SW[0], SW[1] + ("conc_input=h2o.nc", "iprofile=0")), GOOD, '"conc_input" cannot be combined with "scenarios"'),
    "seventeen_inputs": (("lw_spectra", ("input=" + " ".join(["h2o.nc"] * 17),)), "a refused_a.nc" + " asis" * 17 + "\n", "17 input files, 16 at most"),
}


@pytest.mark.parametrize("env", [None, NO_DEVICE], ids=["device", "no_device"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals(files, case, env):
    (tool, keys), table, message = REFUSALS[case]
    d = files["d"]
    sizes = {name: (d / name).stat().st_size for name in ("co2.nc", "gpoints.nc", "ssi.nc", "rayleigh.nc")}
    if table is None:
        if (d / "table.txt").exists():
            (d / "table.txt").unlink()
    else:
        (d / "table.txt").write_text(table)
    r = _tool(tool, *keys, "scenarios=table.txt", cwd=d, env=env)
    assert r.returncode == PARAMETER_ERROR, r.stderr + r.stdout
    assert message in r.stderr, r.stderr
    assert not (d / "refused_a.nc").exists() and not (d / "refused_b.nc").exists()
    assert sizes == {name: (d / name).stat().st_size for name in sizes}        # and no file this run reads was touched


def _same_model(a, b):
    a, b = _nc(a), _nc(b)
    try:
        return set(a.variables) == set(b.variables) and all(np.array_equal(a.variables[k][...], b.variables[k][...]) for k in a.variables)
    finally:
        a.close(); b.close()


def test_chain_trains_the_model_of_the_single_runs(chain):
    """both sides of a training set from one read each: ckdmip_lw --scenarios and lw_spectra gpoints= scenarios= on the same two
    lines, then optimize_lut on their files - the model it writes from the files of the single runs, variable by variable"""
    d = chain
    (d / "sc_lbl.txt").write_text("train sc_lbl_train.nc scale=1.5 asis\nrel sc_lbl_rel.nc asis asis\n")
    (d / "sc_gp.txt").write_text("train sc_gp_train.nc scale=1.5 asis\nrel sc_gp_rel.nc asis asis\n")
    _ok(_tool("ckdmip_lw", "--config", "lw0.nam", "--scenarios", "sc_lbl.txt", "ideal_h2o.nc", "ideal_co2.nc", cwd=d))
    _ok(_tool("lw_spectra", "input=ideal_h2o.nc ideal_co2.nc", "gpoints=gpoints.nc", "scenarios=sc_gp.txt", cwd=d))
    for table_file, single in (("sc_gp_train.nc", "gp0.nc"), ("sc_gp_rel.nc", "gprel.nc")):
        assert _same_model(d / table_file, d / single)
    w = f"gpoint_profile_weight={WEIGHT}"
    _ok(_tool("optimize_lut", "input=raw.nc", "training_input=sc_lbl_train.nc sc_lbl_rel.nc", "gpoint_training_input=sc_gp_train.nc sc_gp_rel.nc",
              w, "output=sc_model.nc", *KEYS, cwd=d))
    _ok(_tool("optimize_lut", "input=raw.nc", "training_input=lbl0.nc lblrel.nc", "gpoint_training_input=gp0.nc gprel.nc", w,
              "output=sc_model_single.nc", *KEYS, cwd=d))
    assert _same_model(d / "sc_model.nc", d / "sc_model_single.nc")
    plain = d / "sc_model_plain.nc"
    _ok(_tool("optimize_lut", "input=raw.nc", "training_input=sc_lbl_train.nc sc_lbl_rel.nc", f"output={plain}", *KEYS, cwd=d))
    assert not _same_model(d / "sc_model.nc", plain)                           # the per-g files did take part
