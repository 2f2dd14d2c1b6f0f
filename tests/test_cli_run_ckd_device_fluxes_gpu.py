"""bin/run_ckd device_gas_optics=1 device_fluxes=1 against the tool with device_gas_optics=1 alone, on a longwave and a shortwave
model (4 columns, 7 layers, ng 16): the flux variables come from the fused call of the handle, everything else from the calls it
came from.  Every non-flux variable is byte-identical; the flux variables, stored as FLOAT, are equal within one float32 ulp of
the larger magnitude.  The key without device_gas_optics=1 is a parameter error."""
import numpy as np
import pytest

import gas_optics_cases as cases
from test_cli_gpu import run_tool
from test_cli_run_ckd_gas_optics_gpu import _files, _read

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sw", [False, True])
def test_device_fluxes_writes_the_same_file(ctx, tmp_path, sw):
    d = tmp_path
    model = (cases.model_sw if sw else cases.model_lw)(ng=16)
    _files(d, model, cases.columns(model, ncol=4, nlay=7))
    r0 = run_tool("run_ckd", "ckd_model=ckd.nc", "input=conc.nc", "output=old.nc", "device_gas_optics=1", cwd=d)
    r1 = run_tool("run_ckd", "ckd_model=ckd.nc", "input=conc.nc", "output=new.nc", "device_gas_optics=1", "device_fluxes=1", cwd=d)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    old, old_att = _read(d / "old.nc")
    new, new_att = _read(d / "new.nc")
    assert list(old) == list(new)
    assert {k: v for k, v in old_att.items() if k != "history"} == {k: v for k, v in new_att.items() if k != "history"}
    assert b"device_fluxes=1" in new_att["history"] and b"device_fluxes" not in old_att["history"]
    fluxes = [k for k in old if "flux" in k]
    assert sorted(fluxes) == (["flux_dn_direct_sw", "spectral_flux_dn_direct_sw"] if sw else
                              ["flux_dn_lw", "flux_up_lw", "spectral_flux_dn_lw", "spectral_flux_up_lw"])
    for k, (code, dims, att, a) in old.items():
        ncode, ndims, natt, b = new[k]
        assert (ncode, ndims, natt) == (code, dims, att) and a.shape == b.shape and code == "f", k
        if k in fluxes:
            ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
            print(k, "values that differ:", int((a != b).sum()), "of", a.size)
            assert np.isfinite(b).all() and a.any() and (np.abs(a - b) <= ulp).all(), k
        else:
            assert a.tobytes() == b.tobytes(), k


def test_device_fluxes_alone_is_a_parameter_error(ctx, tmp_path):
    model = cases.model_lw(ng=16)
    _files(tmp_path, model, cases.columns(model, ncol=4, nlay=7))
    r = run_tool("run_ckd", "ckd_model=ckd.nc", "input=conc.nc", "output=new.nc", "device_fluxes=1", cwd=tmp_path)
    assert r.returncode == 147 and "device_gas_optics=1" in r.stderr, r.stderr + r.stdout        # ECCKD_PARAMETER_ERROR
    assert not (tmp_path / "new.nc").exists()
