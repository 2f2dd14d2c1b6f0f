"""Host-side mirrors of the reference executables' driver logic on top of the C ABI (api.py) and the classic
NetCDF layer (ncio.py).  Only orchestration lives here; every nwav-sized operation runs on the device.

create_look_up_table : src/ecckd/create_look_up_table.cpp:60-606 (without the base_wavenumber_boundary split)
"""
import numpy as np

from . import api, ncio
from ._lib import EcckdError, PARAMETER_ERROR, PROCESSING_ERROR


def _to_device(od, dev):
    """FLOAT on the device when the values are FLOAT (as stored in the CKDMIP files), else DOUBLE: nothing is rounded."""
    import torch
    od32 = od.astype(np.float32)
    return torch.as_tensor(od32 if np.array_equal(od32.astype(np.float64), od) else od, device=dev)


def remove_empty_g_points(g_point, band_number, solar_irradiance=None):
    """create_look_up_table.cpp:111-168: g points that occupy none of the spectrum are dropped and the rest renumbered.
    As in the reference, the new "band_number" of a kept g point is its OLD g-point index (:142), not its band."""
    g_point = np.asarray(g_point)
    ng = int(g_point.max()) + 1
    present = np.zeros(ng, dtype=bool)
    present[g_point[g_point >= 0]] = True
    if present.all():
        return g_point.astype(np.int32), np.asarray(band_number), solar_irradiance
    g_point_map = np.nonzero(present)[0]
    new_g = np.full(g_point.size, -1, dtype=np.int32)
    lookup = np.full(ng, -1, dtype=np.int32)
    lookup[g_point_map] = np.arange(g_point_map.size, dtype=np.int32)
    ok = g_point >= 0
    new_g[ok] = lookup[g_point[ok]]
    if (new_g < 0).any():
        raise EcckdError(1, "Some unassigned spectral points after mapping")          # THROW(1), :146-149
    new_band = g_point_map.copy()
    new_ssi = None if solar_irradiance is None else np.asarray(solar_irradiance)[g_point_map]
    return new_g, new_band, new_ssi


def split_base_g_points(g_point, band_number, band_wn1, band_wn2, base_wavenumber_boundary, wavenumber, ssi, solar_irradiance):
    """create_look_up_table.cpp:160-223: the base (first) g point of every band that contains one of the boundaries is split by
    wavenumber; the g points above move up.  Returns (g_point, band_number, solar_irradiance)."""
    g_point = np.array(g_point, dtype=np.int32)
    band_number = np.array(band_number, dtype=np.int64)
    solar = np.array(solar_irradiance, dtype=np.float64)
    bwb = np.asarray(base_wavenumber_boundary, dtype=np.float64)
    for iband in range(len(band_wn1)):
        inner = bwb[(bwb > band_wn1[iband]) & (bwb < band_wn2[iband])]
        if inner.size == 0:
            continue
        m = inner.size
        ig = int(np.nonzero(band_number == iband)[0].min())
        new_band = np.concatenate([band_number[:ig + 1], np.full(m, iband), band_number[ig + 1:]])
        new_solar = np.concatenate([solar[:ig], np.zeros(m + 1), solar[ig + 1:]])
        bounds = np.concatenate([[band_wn1[iband]], inner, [band_wn2[iband]]])
        old = g_point.copy()
        g_point = np.where(old > ig, old + m, old)
        for k in range(m + 1):
            g_point[(old == ig) & (wavenumber >= bounds[k]) & (wavenumber < bounds[k + 1])] = ig + k
        for k in range(m + 1):
            new_solar[ig + k] = ssi[g_point == ig + k].sum()
        band_number, solar = new_band, new_solar
    return g_point, band_number, solar


def create_look_up_table(ctx, g_point, band_number, band_wn1, band_wn2, gases, averaging_method="transmission",
                         temperature_stride=1, ssi=None, solar_irradiance=None, base_wavenumber_boundary=None, ssi_wavenumber=None):
    """The look-up-table assembly of create_look_up_table.cpp:225-606 from classic NetCDF spectra.

    g_point[nwav], band_number[ng]: from the g-points file (find_g_points' output).
    gases: list of dict(name=..., conc="none"|"linear"|"lut"|"relative-linear", and
             conc == "none":  inputs=[dict(path=..., scaling=-1, conc=-1), ...]  (read_merged_spectrum of the well-mixed files)
             otherwise:       inputs=[path, ...] (one file; one per mole fraction for "lut"), reference_conc for "relative-linear")
    ssi[nwav] selects the shortwave (weights = solar spectral irradiance, :333-340), otherwise Planck weights at each
    layer's temperature (:316-327).  Returns the model dict of api.Optimizer / ncio.write_ckd_model."""
    import torch
    is_sw = ssi is not None
    ng_file = int(np.asarray(g_point).max()) + 1
    g_point, band_number, solar_irradiance = remove_empty_g_points(g_point, band_number, solar_irradiance)
    save_g_points = int(g_point.max()) + 1 != ng_file                     # the numbering left the g-points file's (:575-577)
    if base_wavenumber_boundary is not None and len(base_wavenumber_boundary) > 0:
        if not is_sw or ssi_wavenumber is None:
            raise EcckdError(PARAMETER_ERROR, "base_wavenumber_boundary needs the ssi file (its wavenumbers and irradiances)")
        g_point, band_number, solar_irradiance = split_base_g_points(g_point, band_number, band_wn1, band_wn2, base_wavenumber_boundary,
                                                                      np.asarray(ssi_wavenumber), np.asarray(ssi), solar_irradiance)
        save_g_points = True
    ng = int(g_point.max()) + 1
    dev = ctx.device
    d_ssi = torch.as_tensor(np.asarray(ssi, dtype=np.float64), device=dev) if is_sw else None
    gmap = hr_wavenumber = None
    model = dict(gases=[], iband_per_g=np.asarray(band_number, dtype=np.int32))
    temperature_fl = None

    def column(s, od_dev, ref_vmr):
        nonlocal gmap, temperature_fl, hr_wavenumber
        p, t = s["pressure_hl"], s["temperature_hl"]
        if gmap is None:
            wn = torch.as_tensor(s["wavenumber_cm_1"], device=dev)
            dwn = torch.as_tensor(s["d_wavenumber_cm_1"], device=dev)
            gmap = api.GPointMap(ctx, torch.as_tensor(g_point, device=dev), ng, wn, dwn)
            hr_wavenumber = np.asarray(s["wavenumber_cm_1"], dtype=np.float64)
            model["log_pressure"] = np.log(0.5 * (p[1:] + p[:-1]))
        t_fl = (t[:-1] * p[:-1] + t[1:] * p[1:]) / (p[:-1] + p[1:])                  # :310-311
        out = gmap.average_optical_depth(p, od_dev, averaging_method, reference_surface_vmr=ref_vmr,
                                         temperature_fl=None if is_sw else t_fl, ssi=d_ssi)
        return t_fl, out

    for spec in gases:
        name, conc = spec["name"], spec["conc"]
        if conc not in ("none", "linear", "lut", "relative-linear"):
            raise EcckdError(PARAMETER_ERROR, f'conc_dependence "{conc}" not understood')
        g = dict(name=name, conc=conc, active=True)
        files = spec["inputs"]
        nconc = len(files) if conc == "lut" else 1
        tables, vmrs, tfl_rows = None, [], None
        for iconc in range(nconc):
            ncol, icol = 1, 0
            while icol < ncol:
                if conc == "none":
                    # read_merged_spectrum (:293-296): sum of the scaled well-mixed spectra, accumulated on the device
                    merged, first = None, None
                    ci = spec.get("conc_input")                          # dict(path, iprofile): read_merged_spectrum.cpp:47-61
                    rows_vmr, mols = [], []
                    for item in files:
                        s = ncio.read_spectrum(item["path"], icol * temperature_stride)
                        first = first or s
                        pc = cr = None
                        if ci is not None:
                            with ncio.NcFile(ci["path"]) as cf:
                                pc = cf.read("pressure_fl", ci["iprofile"])
                                cr = cf.read(s["molecule"].split(" ")[0] + "_mole_fraction_fl", ci["iprofile"])
                        sp, vrow = api.merge_scaling(s["pressure_hl"], item.get("scaling", -1.0), item.get("conc", -1.0),
                                                     s["reference_surface_vmr"], s["vmr_fl"], pressure_conc=pc, conc_req=cr)
                        rows_vmr.append(vrow); mols.append(s["molecule"])
                        merged = api.merge_spectrum(ctx, _to_device(s["optical_depth"], dev), sp, merged)
                    if icol == 0:                                         # create_look_up_table.cpp:311-313
                        g["composite_vmr"], g["composite_molecules"] = np.stack(rows_vmr), " ".join(mols)
                    s, od_dev, ref_vmr = first, merged, 1.0                            # reference_surface_vmr = 1 (:283)
                else:
                    s = ncio.read_spectrum(files[iconc], icol * temperature_stride)
                    od_dev = _to_device(s["optical_depth"], dev)
                    ref_vmr = s["reference_surface_vmr"]
                    if conc == "lut" and ref_vmr < 0.0:
                        raise EcckdError(PARAMETER_ERROR, "Invalid reference_surface_vmr for constructing VMR-dependent look-up table")
                ncol = (s["ncol"] + temperature_stride - 1) // temperature_stride
                t_fl, (k, kmin, kmax) = column(s, od_dev, ref_vmr)
                if tables is None:
                    shape = (nconc, ncol) + k.shape
                    tables = [np.zeros(shape) for _ in range(3)]
                    tfl_rows = np.zeros((ncol, k.shape[0]))
                for tab, v in zip(tables, (k, kmin, kmax)):
                    tab[iconc, icol] = v
                tfl_rows[icol] = t_fl
                icol += 1
            if conc == "lut":
                vmrs.append(ref_vmr)
        temperature_fl = tfl_rows                                                     # the last gas's, as the reference keeps it
        squeeze = (lambda a: a) if conc == "lut" else (lambda a: a[0])
        g["molar_abs"], g["min_molar_abs"], g["max_molar_abs"] = (squeeze(t) for t in tables)
        if conc == "lut":
            g["vmr"] = np.array(vmrs)
        if conc == "relative-linear":
            if "reference_conc" not in spec:
                raise EcckdError(PARAMETER_ERROR, f"{name}.reference_conc must be provided if conc_dependence is relative-linear")
            g["reference_vmr"] = float(spec["reference_conc"])
        model["gases"].append(g)

    model["temperature"] = temperature_fl
    # fraction of the spectrum contributing to each g point on a 10 (LW) / 50 (SW) cm-1 grid (:507-548)
    dwav = 50 if is_sw else 10
    startwav = int(np.floor(np.min(band_wn1) / dwav) * dwav)
    endwav = int(np.ceil(np.max(band_wn2) / dwav) * dwav)
    model["wavenumber1"] = dwav * np.arange(startwav // dwav, endwav // dwav, dtype=np.float64)
    model["wavenumber2"] = dwav * np.arange(startwav // dwav + 1, endwav // dwav + 1, dtype=np.float64)
    model["gpoint_fraction"] = gmap.gpoint_fraction(model["wavenumber1"], model["wavenumber2"])
    model["wavenumber1_band"], model["wavenumber2_band"] = np.asarray(band_wn1, float), np.asarray(band_wn2, float)
    model["nband"] = len(model["wavenumber1_band"])
    if is_sw:
        model["solar_irradiance"] = np.asarray(solar_irradiance, dtype=np.float64)
        model["planck_function"] = model["temperature_planck"] = None
        # solar irradiance of each interval (:556-561) and the Rayleigh coefficient of each g point
        # (CkdModel::calc_rayleigh_molar_scat, ckd_model.h:368-385; Bucholtz 1995, rayleigh_scattering.h:25-43)
        w1, w2, ssi64 = model["wavenumber1"], model["wavenumber2"], np.asarray(ssi, dtype=np.float64)
        k = np.searchsorted(w2, hr_wavenumber, side="left")                 # wavenumber1 < w <= wavenumber2
        ok = (k < w2.size) & (hr_wavenumber > w1[np.minimum(k, w1.size - 1)])
        model["solar_spectral_irradiance"] = np.bincount(k[ok], weights=ssi64[ok], minlength=w1.size)
        um = 10000.0 / (0.5 * (w1 + w2))
        xs = np.where(um < 0.5, 3.01577e-32 * um ** -(3.55212 + 1.35579 * um + 0.11563 / um),
                      4.01061e-32 * um ** -(3.99668 + 0.00110298 * um + 0.0271393 / um))
        molar_column = 1.0e5 / (9.80665 * 0.001 * 28.970)
        trans_hr = np.exp(-molar_column * xs * 6.02214076e23 / 0.5)
        gf, si = model["gpoint_fraction"], model["solar_spectral_irradiance"]
        model["rayleigh_molar_scattering"] = -np.log(np.maximum(1.0e-14, (gf @ (si * trans_hr)) / (gf @ si))) * 0.5 / molar_column
    else:
        model["temperature_planck"] = np.arange(120.0, 351.0)                         # :581
        model["planck_function"] = gmap.planck_lut(model["temperature_planck"])        # :585-591
    model["ng"] = ng
    if save_g_points:
        model["save_g_points"], model["wavenumber_hr"], model["g_point_hr"] = True, hr_wavenumber, g_point
    gmap.close()
    return model


def iband_per_g(model, wavenumber1, wavenumber2):
    """CkdModel::iband_per_g (ckd_model.h:287-306): the LBL band each g point lies in, from gpoint_fraction."""
    gf, w1, w2 = np.asarray(model["gpoint_fraction"]), np.asarray(model["wavenumber1"]), np.asarray(model["wavenumber2"])
    iband = np.full(gf.shape[0], -1, dtype=np.int32)
    for ib in range(len(wavenumber1)):
        weight = gf[:, (w1 >= wavenumber1[ib]) & (w2 <= wavenumber2[ib])].sum(axis=1)
        if np.any((weight > 0.05) & ((weight < 0.95) | (weight > 1.05))):
            raise EcckdError(1, "G-points do not lie entirely within requested bands")
        iband[weight > 0.5] = ib
    if np.any(iband < 0):
        raise EcckdError(1, "Some g-points not inside a band")
    return iband


def optimize_lut(ctx, model, training_files, relative_to=None, band_mapping=None, gmap=None, max_iterations=3000,
                 convergence_criterion=0.0, bounded=True, max_no_rayleigh_wavenumber=None, erythemal_weight=0.0,
                 remove_min_max=False, rayleigh_scattering=False, optimize_rayleigh=False, rayleigh_prior_error=0.0, nangle=0,
                 gpoint_training_input=None, gpoint_relative_to=None, gpoint_profile_weight=0.0, **cfg):
    """The driver of optimize_lut.cpp:60-330 on top of api.Optimizer: training scenes from LBL flux files
    (ncio.read_lbl_fluxes), optional "relative_to" file, bounded L-BFGS, optimised coefficients back into the model.

    model: dict from ncio.read_ckd_model (its `active` flags select the gases being optimised, optimize_lut.cpp:161).
    cfg:   flux_weight, flux_profile_weight, broadband_weight, spectral_boundary_weight, prior_error, ... (api.Optimizer).
    remove_min_max: drop the min / max tables from the model that is returned (`ckd_model.save_min_max(false)`,
           optimize_lut.cpp:243-244, :308-310), so that ncio.write_ckd_model leaves the _min / _max variables out.
    rayleigh_scattering: train through the two-stream transfer with Rayleigh scattering (api.Optimizer(rayleigh_scattering=True),
           the tool's key of the same name): every file must be a `ckdmip_sw --rayleigh` one, the truth's downwelling is the
           total flux, nothing is masked (max_no_rayleigh_wavenumber is ignored) and relative_to goes through a scattering
           handle as well.
    optimize_rayleigh: the ng Rayleigh coefficients are optimised too (api.Optimizer(optimize_rayleigh=True), the tool's key of
           the same name), with either forward model; rayleigh_prior_error is the sigma of their prior (<= 0: none).  Every
           gas of the model may then be inactive.  The relative_to handle is made without it.  The model that is returned
           carries the optimised rayleigh_molar_scattering.
    nangle: N in 1..16: train a longwave model under the zenith-angle quadrature the truth files were made with (`ckdmip_lw` with
           nangle = N; api.Optimizer(nangle=N), the tool's key of the same name), for the relative_to handle as well; 0: the
           two-stream form.  A file that carries a global attribute `nangle` must agree with the key.
    gpoint_training_input, gpoint_profile_weight: the per-g flux-profile term (Optimizer.set_gpoint_truth; the tool's keys of the
           same names, none of them the reference's): one `lw_spectra gpoints=` file per training file, in the same order, and the
           weight of the term; both or neither.  gpoint_relative_to: the per-g truth of the relative_to scene, given exactly when
           relative_to is; it is subtracted from every file's truth.  Longwave models only.  Every file must hold the model's g
           points, the columns, half levels and (to 1e-5) pressures of its training file, and the nangle of the key nangle (a
           file without the attribute counts as 0).
    Returns (model with optimised molar_abs, result dict of Optimizer.minimize)."""
    names = [g["name"] for g in model["gases"]]
    is_sw = model.get("solar_irradiance") is not None
    gp_files = list(gpoint_training_input) if gpoint_training_input else []
    gp_weight = float(gpoint_profile_weight)
    if gp_weight > 0.0 and not gp_files:
        raise EcckdError(PARAMETER_ERROR, "gpoint_profile_weight > 0 needs gpoint_training_input")
    if gp_files and not gp_weight > 0.0:
        raise EcckdError(PARAMETER_ERROR, "gpoint_training_input needs gpoint_profile_weight > 0")
    if gp_files:
        if len(gp_files) != len(list(training_files)):
            raise EcckdError(PARAMETER_ERROR, f"gpoint_training_input names {len(gp_files)} files, training_input {len(list(training_files))}")
        if is_sw:
            raise EcckdError(PARAMETER_ERROR, "gpoint_training_input needs a longwave CKD model")
        if relative_to is not None and gpoint_relative_to is None:
            raise EcckdError(PARAMETER_ERROR, "relative_to with gpoint_training_input needs gpoint_relative_to")
    if gpoint_relative_to is not None and (relative_to is None or not gp_files):
        raise EcckdError(PARAMETER_ERROR, "gpoint_relative_to needs relative_to and gpoint_training_input")
    if rayleigh_scattering and not (is_sw and model.get("rayleigh_molar_scattering") is not None):
        raise EcckdError(PARAMETER_ERROR, "rayleigh_scattering needs a shortwave CKD model with a Rayleigh coefficient")
    if optimize_rayleigh and not (is_sw and model.get("rayleigh_molar_scattering") is not None):
        raise EcckdError(PARAMETER_ERROR, "optimize_rayleigh needs a shortwave CKD model with a Rayleigh coefficient")
    nangle = int(nangle)
    if not 0 <= nangle <= 16:
        raise EcckdError(PARAMETER_ERROR, f"nangle = {nangle} outside 0..16")
    if nangle > 0 and is_sw:
        raise EcckdError(PARAMETER_ERROR, f"nangle = {nangle} needs a longwave CKD model")
    for path in ([relative_to] if relative_to is not None else []) + list(training_files):
        file_nangle = ncio.lbl_fluxes_nangle(path)
        if file_nangle is not None and file_nangle != nangle:
            raise EcckdError(PARAMETER_ERROR, f"{path} was made with nangle = {file_nangle}, the key nangle says {nangle}")

    def load(path):
        s = ncio.read_lbl_fluxes(path, names, band_mapping=band_mapping, gmap=gmap, ctx=ctx, rayleigh_scattering=rayleigh_scattering)
        if s["have_band_fluxes"]:
            s["iband_per_g"] = iband_per_g(model, s["band_wavenumber1"], s["band_wavenumber2"])     # :273-276
        if is_sw and max_no_rayleigh_wavenumber is not None and not rayleigh_scattering:
            ncio.mask_rayleigh_up(s, max_no_rayleigh_wavenumber)                                     # :278-283
        if is_sw and erythemal_weight > 0.0 and "erythemal_spectrum" in s:
            s["spectral_boundary_weights"] = erythemal_weight * s["erythemal_spectrum"]              # solve_adept.cpp:182
        return s

    rel = None
    if relative_to is not None:                                                                      # :204-236
        rel = load(relative_to)
        m0 = dict(model, iband_per_g=rel.get("iband_per_g", model["iband_per_g"]))
        if not any(g.get("active", True) for g in model["gases"]):     # Rayleigh alone: this handle, made without the flag, takes every gas
            m0["gases"] = [dict(g, active=True) for g in model["gases"]]
        ref_opt = api.Optimizer(ctx, m0, [_scene_for_optimizer(rel, is_sw)], rayleigh_scattering=rayleigh_scattering, nangle=nangle,
                                **cfg)
        _, fl = ref_opt.forward(ref_opt.initial_state(), unclamped=True)     # od = value(aod), no clamp (:231-234)
        ref_opt.close()
    def load_gpoints(path, like):
        # the per-g truth of the scene `like`, checked against it, the model and the key nangle
        try:
            t = ncio.read_gpoint_fluxes(path)
        except ValueError as exc:
            raise EcckdError(PARAMETER_ERROR, str(exc))
        ng = int(np.asarray(model["iband_per_g"]).size)
        if t["flux"].shape[3] != ng:
            raise EcckdError(PARAMETER_ERROR, f"{path} has {t['flux'].shape[3]} g points, the CKD model {ng}")
        p = np.asarray(like["pressure_hl"], dtype=np.float64)
        if t["pressure_hl"].shape != p.shape:
            raise EcckdError(PARAMETER_ERROR, f"{path} has (columns, half levels) = {t['pressure_hl'].shape}, its training file {p.shape}")
        if np.any(np.abs(t["pressure_hl"] - p) > 1e-5 * np.abs(p)):
            raise EcckdError(PARAMETER_ERROR, f"{path}: pressure_hl differs from its training file's by more than 1e-5")
        if t["nangle"] != nangle:
            raise EcckdError(PARAMETER_ERROR, f"{path} was made with nangle = {t['nangle']}, the key nangle says {nangle}")
        return t["flux"]

    gp_rel = load_gpoints(gpoint_relative_to, rel) if gpoint_relative_to is not None else None
    gp_truth = []
    scenes = []
    iband = None
    for ifile, path in enumerate(training_files):
        s = load(path)
        if gp_files:
            t = load_gpoints(gp_files[ifile], s)
            if gp_rel is not None:
                if gp_rel.shape != t.shape:
                    raise EcckdError(PARAMETER_ERROR, f"{gp_files[ifile]} and {gpoint_relative_to} differ in shape: {t.shape}, {gp_rel.shape}")
                t = t - gp_rel
            gp_truth.append(t)
        if rel is not None:
            ncio.subtract_lbl_fluxes(s, rel)                                                         # :251-254
        sc = _scene_for_optimizer(s, is_sw)
        if rel is not None:
            sc["relative_flux_dn"], sc["relative_flux_up"] = np.ascontiguousarray(fl[:, 0]), np.ascontiguousarray(fl[:, 1])
        scenes.append(sc)
        iband = s.get("iband_per_g", iband)
    if not scenes:
        raise EcckdError(PARAMETER_ERROR, '"training_input" not specified')
    m = dict(model)
    if iband is not None:
        m["iband_per_g"] = iband
    opt = api.Optimizer(ctx, m, scenes, rayleigh_scattering=rayleigh_scattering, optimize_rayleigh=optimize_rayleigh,
                        rayleigh_prior_error=rayleigh_prior_error, nangle=nangle,
                        gpoint_truth=np.concatenate(gp_truth, axis=0) if gp_truth else None, gpoint_profile_weight=gp_weight,
                        **dict(dict(cap_relative_linear=0.8), **cfg))   # :185
    res = opt.minimize(max_iterations=max_iterations, convergence_criterion=convergence_criterion, bounded=bounded)
    out = dict(model, gases=[dict(g) for g in model["gases"]])
    for i, g in enumerate(out["gases"]):
        g["molar_abs"] = opt.coefficients(res["x"], i, np.asarray(g["molar_abs"]).shape)
        if remove_min_max:
            g.pop("min_molar_abs", None)
            g.pop("max_molar_abs", None)
    if optimize_rayleigh:
        out["rayleigh_molar_scattering"] = opt.rayleigh_coefficients(res["x"])
    opt.close()
    return out, res


def _scene_for_optimizer(s, is_sw):
    keys = ["pressure_hl", "temperature_hl", "vmr_fl", "gas_present", "flux_dn", "flux_up", "spectral_flux_dn_surf",
            "spectral_flux_up_toa", "spectral_boundary_weights"]
    if is_sw:
        keys += ["mu0", "tsi", "albedo"]
    return {k: s[k] for k in keys if s.get(k) is not None}


def reorder_spectrum(ctx, input_path, output_path, band_bound1, band_bound2, iprofile=0, threshold_optical_depth=None,
                     ssi=None, config_str="", history=None):
    """reorder_spectrum.cpp:45-310 for one gas: spectrum file in, reordering file out.  Returns the order dict."""
    s = ncio.read_spectrum(input_path, iprofile)
    thr = threshold_optical_depth if threshold_optical_depth is not None else (0.5 if ssi is None else 0.25)
    od = s["optical_depth"]
    od32 = od.astype(np.float32)
    od_in = od32 if np.array_equal(od32.astype(np.float64), od) else od
    key, col, iband, rank = api.reorder_spectrum(ctx, s["pressure_hl"], s["wavenumber_cm_1"], s["d_wavenumber_cm_1"], od_in, ssi, thr,
                                                 band_bound1, band_bound2)
    # the file stores the bounds clamped to the range of the data (reorder_spectrum.cpp:268-273)
    wn = s["wavenumber_cm_1"]
    band_bound1, band_bound2 = np.array(band_bound1, dtype=np.float64), np.array(band_bound2, dtype=np.float64)
    band_bound1[0], band_bound2[-1] = max(wn[0], band_bound1[0]), min(wn[-1], band_bound2[-1])
    ncio.write_order(output_path, band_bound1, band_bound2, s["wavenumber_cm_1"], s["d_wavenumber_cm_1"], iband, rank, key, col,
                     molecule=s["molecule"] or "", config_str=config_str, history=history)
    return dict(spectrum=s, key=key, column_optical_depth=col, band_number=iband, rank=rank)


def reorder_cloud_spectrum(ctx, input_path, wavenumber_input, output_path, isize, band_bound1=None, band_bound2=None, config_str="",
                           history=None):
    """reorder_cloud_spectrum.cpp:31-201: the optically thick absorptance of size bin `isize` of a Mie scattering file on the grid
    of `wavenumber_input`, ranked per band, written as the reordering file of the cloud pseudo-gas.  Returns the order dict."""
    import torch
    with ncio.NcFile(wavenumber_input) as f:
        wn = f.read("wavenumber")
    with ncio.NcFile(input_path) as f:
        cloud_wn = f.read("wavenumber")
        nsize = f.var_info("single_scattering_albedo")[1][0]
        if not 0 <= isize < nsize:
            raise EcckdError(PARAMETER_ERROR, "isize = %d is outside the %d size bins of %s" % (isize, nsize, input_path))
        ssa = f.read("single_scattering_albedo", isize)
        asymmetry = f.read("asymmetry_factor", isize)
    d_wn = torch.as_tensor(wn, device=ctx.device)
    dwn = api.derive_d_wavenumber(ctx, d_wn).cpu().numpy()                                                  # :86-92
    if band_bound1 is None:                                                                                 # :132-137
        band_bound1, band_bound2 = [max(0.0, wn[0] - dwn[0])], [wn[-1] + dwn[-1]]
    band_bound1, band_bound2 = np.array(band_bound1, dtype=np.float64), np.array(band_bound2, dtype=np.float64)
    key = api.cloud_sorting_variable(ctx, cloud_wn, ssa, asymmetry, d_wn)
    iband, bb, be = api.band_ranges(wn, band_bound1, band_bound2)
    if np.any(bb > be):
        raise EcckdError(PARAMETER_ERROR, "reorder_cloud_spectrum: band %d contains no wavenumbers" % int(np.nonzero(bb > be)[0][0]))
    rank, _ = api.stable_argsort_bands(ctx, key, bb, be, want_ordered=False)
    key, rank = key.cpu().numpy(), rank.cpu().numpy()
    band_bound1[0], band_bound2[-1] = max(wn[0], band_bound1[0]), min(wn[-1], band_bound2[-1])              # :156-161
    ncio.write_order(output_path, band_bound1, band_bound2, wn, dwn, iband, rank, key, None, molecule="cloud", config_str=config_str,
                     history=history)
    return dict(wavenumber=wn, d_wavenumber=dwn, sorting_variable=key, band_number=iband, rank=rank,
                wavenumber1_band=band_bound1, wavenumber2_band=band_bound2)


def cloud_g_points(ctx, cloud, ssi, nwav=None, nband=None):
    """find_g_points.cpp:543-652: the single-gas g points of the cloud pseudo-gas.
    cloud: dict(name, reordering_input, max_reflectance_range=0.26).  nwav / nband: those of the gases, checked."""
    import torch
    order = ncio.read_order(cloud["reordering_input"])
    iband = order["band_number"]
    nb = order["wavenumber1_band"].size
    if (nwav is not None and iband.size != nwav) or (nband is not None and nb != nband) or len(ssi) != iband.size:
        raise EcckdError(PARAMETER_ERROR, "The ordering of %s has %d wavenumbers in %d bands, the gases %s in %s" %
                         (cloud["name"], iband.size, nb, nwav, nband))
    bb, be = _band_index_ranges(iband, nb)
    dev = ctx.device
    rank = torch.as_tensor(order["rank"], device=dev)
    res = api.cloud_partition(ctx, torch.as_tensor(np.asarray(ssi, dtype=np.float64), device=dev), rank,
                              torch.as_tensor(order["sorting_variable"], device=dev), bb, be,
                              cloud.get("max_reflectance_range", 0.26))
    gp = api.gas_g_point(ctx, rank, res["rank1"], res["rank2"])
    out = dict(name=cloud["name"], n_g_points=[int(v) for v in res["n_g_points"]], band_number=[int(v) for v in res["band_number"]],
               rank1=[int(v) for v in res["rank1"]], rank2=[int(v) for v in res["rank2"]], error=[float(v) for v in res["error"]],
               sorting_variable=[float(v) for v in res["median"]], status=[], comp_cost=[])
    return out, gp


def _band_index_ranges(iband, nband):
    """First / last index of every band of a band_number array (-1, -1 for an empty band)."""
    bb, be = np.full(nband, -1, dtype=np.int64), np.full(nband, -1, dtype=np.int64)
    for b in range(nband):
        idx = np.nonzero(iband == b)[0]
        if idx.size:
            bb[b], be[b] = idx[0], idx[-1]
    return bb, be


def reorder_single_band_sharded(ctx, pressure_hl, wn, dwn, od, threshold_optical_depth=0.5, group=None):
    """reorder_spectrum of ONE longwave band (the fsck structure) with the key sweep split by wavenumber range over the processes
    of `group`: every process runs K1 on its own whole-tile range of the resident spectrum, the keys and column
    optical depths travel to rank 0 once (16 B per wavenumber), rank 0 runs the one stable sort (K3).  A wavenumber's key is a
    function of its column alone, so key, column optical depth and rank have the bits one process gives.
    -> (key, col_od, rank) device tensors on rank 0, (None, None, None) elsewhere."""
    from . import shard
    t_ideal = api.idealised_temperature(pressure_hl)
    nwav = od.shape[1]

    def key_of_range(b, e):
        if e <= b:
            import torch
            z = torch.empty(0, dtype=torch.float64, device=ctx.device)
            return z, z
        key, col = api.reorder_key_lw(ctx, pressure_hl, t_ideal, wn[b:e], dwn[b:e], od[:, b:e], threshold_optical_depth)
        ctx.synchronize()
        return key, col

    def sort_on_root(key):
        rnk, _ = api.stable_argsort_bands(ctx, key, [0], [nwav - 1], want_ordered=False)
        return rnk

    return shard.reorder_single_band(key_of_range, nwav, sort_on_root, group=group, device=ctx.device)


def _prepare_gas(ctx, g, averaging_method, flux_weight, min_pressure, planck_reuse=None, sw=None):
    """Gas preparation (find_g_points.cpp:872-1150) of one gas whose spectra are on the device, and its sorting variable in
    sorted order (:781).  g, sw, planck_reuse: see _search_gas.  -> (gas handle, sorting variable sorted, band albedo or None)"""
    import time
    timing = g.setdefault("timing", {})
    t0 = time.perf_counter()
    if sw is None:
        # the background as the merged matrix "bg", or as the spectra it is merged from, "bg_sources" (api.GasLW)
        gas = api.GasLW(ctx, g["pressure_hl"], g["temperature_hl"], g["wn"], g["dwn"], g["rank"], g["od"], g.get("bg"),
                        averaging_method, flux_weight, min_pressure, planck_hl_reuse=planck_reuse, bg_sources=g.get("bg_sources"))
        band_albedo = None
    else:
        gas = api.GasSW(ctx, g["pressure_hl"], sw["ssi"], g["rank"], g["od"], g.get("bg"), averaging_method, flux_weight,
                        min_pressure, sw["cos_sza"], sw["albedo"], g.get("min_scaling", 1.0), g.get("max_scaling", 1.0))
        band_albedo = sw["band_albedo"]
    sv_sorted = api.gather_f64(ctx, g["sorting_variable"], api.invert_permutation(ctx, g["rank"]))
    ctx.synchronize()
    timing["preparation"] = timing.get("preparation", 0.0) + time.perf_counter() - t0
    return gas, sv_sorted, band_albedo


def _band_requests(g, bands, tol, band_albedo):
    """The arguments of ecckd_find_g_bands_ex for `bands` of gas g: first / last sorted index, tolerance and options per band;
    a shortwave band brings its albedo (init_sw(..., band_albedo(jband), ...)) with it."""
    begin, end = g["band_begin"], g["band_end"]
    opts = [dict(min_g_points=int(g["min_g_points"][b]), max_g_points=int(g["max_g_points"][b])) for b in bands]
    if band_albedo is not None:
        opts = [dict(o, band_albedo=float(band_albedo[b])) for b, o in zip(bands, opts)]
    return dict(ibegin=[int(begin[b]) for b in bands], iend=[int(end[b]) for b in bands],
                heating_rate_tolerance=np.ascontiguousarray(np.asarray(tol)[bands]), options=opts)


def _finish_gas(gas, g, bands, band_res, sv_sorted):
    """The median sorting variable of every g point of these bands in one call (:1404-1409) and the per-band result dicts."""
    import time
    t2 = time.perf_counter()
    r1_all = np.concatenate([np.asarray(res["rank1"], dtype=np.int64) for res in band_res])
    r2_all = np.concatenate([np.asarray(res["rank2"], dtype=np.int64) for res in band_res])
    med_all = gas.median_sorting_variable(sv_sorted, r1_all, r2_all)
    out = []
    k0 = 0
    for b, res in zip(bands, band_res):
        n = len(res["rank1"])
        med = med_all[k0:k0 + n]
        k0 += n
        out.append((b, dict(rank1=[int(v) for v in res["rank1"]], rank2=[int(v) for v in res["rank2"]],
                            error=[float(v) for v in res["error"]], status=int(res["status"]),
                            comp_cost=float(res["comp_cost"]), sorting_variable=[float(v) for v in med])))
    timing = g.setdefault("timing", {})
    timing["medians"] = timing.get("medians", 0.0) + time.perf_counter() - t2
    return out


def _search_gas(ctx, g, bands, tol, tolerance_tolerance, max_iterations, averaging_method, flux_weight, min_pressure,
                sequential_bands, planck_reuse=None, sw=None):
    """One gas of the loop find_g_points.cpp:655-1450 with everything already on the device: gas preparation (:872-1150),
    the searches of `bands` (:1152-1414, side by side unless sequential_bands) and the median sorting variable of every
    g point (:1404-1409).

    g:  dict(pressure_hl, temperature_hl (host), wn, dwn, rank (int32), od, bg (or None), sorting_variable: device tensors in
        ORIGINAL wavenumber order; band_begin[nband], band_end[nband]: first / last sorted index of every band;
        min_g_points[nband], max_g_points[nband]; shortwave: min_scaling, max_scaling)
    sw: None (longwave; planck_reuse = device pointer of the first gas's Planck matrix or None) or
        dict(ssi, albedo: device tensors, band_albedo[nband], cos_sza).
    Returns (gas handle - the caller closes it -, [(band, dict(rank1, rank2, error, status, comp_cost, sorting_variable))])."""
    import time
    gas, sv_sorted, band_albedo = _prepare_gas(ctx, g, averaging_method, flux_weight, min_pressure, planck_reuse, sw)
    timing = g["timing"]
    t1 = time.perf_counter()
    req = _band_requests(g, bands, tol, band_albedo)
    if len(bands) > 1 and not sequential_bands:
        # bands side by side, sharing their error batches (ecckd_find_g_bands_ex): same decisions per band
        band_res = gas.find_g_bands_ex(req["ibegin"], req["iend"], req["heating_rate_tolerance"], tolerance_tolerance, max_iterations,
                                       req["options"])
    else:
        band_res = []
        for k, b in enumerate(bands):
            o = dict(req["options"][k])
            o.pop("band_albedo", None)
            if band_albedo is not None:
                gas.set_band_albedo(band_albedo[b])                                                   # init_sw(..., band_albedo(jband), ...)
            band_res.append(gas.find_g_band_ex(req["ibegin"][k], req["iend"][k], float(tol[b]), tolerance_tolerance, max_iterations, **o))
    timing["search"] = timing.get("search", 0.0) + time.perf_counter() - t1
    return gas, _finish_gas(gas, g, bands, band_res, sv_sorted)


def _deal(ngas, nband, rank, world_size, group):
    from . import shard
    if rank is None or world_size is None:
        rank, world_size = shard.world(group)
    tasks = shard.task_table(range(ngas), nband)
    mine = [tasks[t] for t in shard.deal_tasks(len(tasks), rank, world_size)]
    my_bands = {}
    for gi, b in mine:
        my_bands.setdefault(gi, []).append(b)
    return rank, world_size, tasks, mine, my_bands


def _collect(local, ntasks, rank, world_size, group, dev):
    """The only communication of a sharded find_g_points: the per-band results to rank 0, ONE all-reduce of the final cost
    (sum of the g points' errors) and of the work counter."""
    from . import shard
    cost_local = float(sum(sum(r["error"]) for _, _, r in local))
    comp_local = float(sum(r["comp_cost"] for _, _, r in local))
    gathered = shard.gather_to_root(local, group)
    if world_size > 1:
        _, comp_sum, cost_sum = shard.reduce_scalars(0.0, comp_local, cost_local, device=dev if _is_nccl(group) else None, group=group)
    else:
        comp_sum, cost_sum = comp_local, cost_local
    by_task = None
    if rank == 0:
        by_task = {(gi, b): r for part in gathered for gi, b, r in part}
        if len(by_task) != ntasks:
            raise EcckdError(PROCESSING_ERROR, "find_g_points: %d of %d (gas, band) searches came back" % (len(by_task), ntasks))
    return by_task, cost_sum, comp_sum


def _per_gas_tables(names, nband, by_task):
    """SingleGasData of every gas (single_gas_data.h:24-80) from the per-band results, bands in order."""
    per_gas = []
    for gi, name in enumerate(names):
        out = dict(name=name, n_g_points=[], band_number=[], rank1=[], rank2=[], error=[], sorting_variable=[], status=[], comp_cost=[])
        for b in range(nband):
            r = by_task[(gi, b)]
            n = len(r["error"])
            out["n_g_points"].append(n)
            out["band_number"] += [b] * n
            out["rank1"] += r["rank1"]; out["rank2"] += r["rank2"]; out["error"] += r["error"]
            out["sorting_variable"] += r["sorting_variable"]
            out["status"].append(r["status"]); out["comp_cost"].append(r["comp_cost"])
        per_gas.append(out)
    return per_gas


def find_g_points(ctx, gases, band_bound1, band_bound2, heating_rate_tolerance, output_path=None, averaging_method="transmission",
                  flux_weight=0.02, min_pressure=0.0, tolerance_tolerance=0.02, max_iterations=60, iprofile=0, ssi=None,
                  max_no_rayleigh_wavenumber=10000.0, reference_albedo=0.15, cos_sza=0.5, sequential_bands=False,
                  rank=None, world_size=None, group=None, cloud=None, target_g_points=None, target_resolution=1e-3,
                  target_max_trials=40, target_exact=False):
    """The main loop of find_g_points.cpp:655-1660 over classic files (shortwave when `ssi[nwav]` is given: solar weights,
    reference albedo 0.15 below max_no_rayleigh_wavenumber (:469, :522, :757-761, :921-923), REFERENCE_COS_SZA = 0.5,
    per-gas min_scaling / max_scaling (:661-667)): per gas the merged background, the gas
    preparation, the band searches and the median sorting variables; then the overlap of the gases' g points, the merged
    g-point map and the g-points file.

    gases: list of dict(name, input=spectrum file, reordering_input=order file, background=[dict(path, scaling, conc), ...],
                        min_g_points=1, max_g_points=256).

    Several processes (one per GPU, torch.distributed initialised - RCCL on the GPU box - or explicit rank / world_size):
    the (gas, band) searches are independent problems (:655, :1152) and are dealt to the processes as contiguous shares of
    the task table (shard.deal_tasks); a process reads and prepares only the gases of which it searches a band.  Nothing is
    exchanged while searching.  The per-band results (a few numbers per g point) are gathered on rank 0, which does what
    follows the gas loop in the reference (:1452-1660: overlap, merged map, file); ONE all-reduce combines the final cost
    (sum of the g points' errors) and the work counters.  Returns the result dict on rank 0, a summary elsewhere; both hold
    `cost_sum` and `comp_cost_sum`, identical on every rank.  The g points do not depend on the number of processes.

    cloud: None, or (shortwave only) dict(name, reordering_input, max_reflectance_range=0.26): the cloud pseudo-gas of :543-652,
    partitioned by rank 0 after the gases' searches and the first constituent of the overlap (:1448-1451).

    target_g_points: None, or the number of g points wanted (the tool's target_g_points key).  heating_rate_tolerance is then the
    first guess and fixes the ratio between the bands: every gas is prepared first and stays resident, and one call
    (api.find_g_gases_target) searches all of them again and again with the tolerances multiplied by one factor until the
    overlap has that many g points (target_resolution, target_max_trials: the bounds of that search; target_exact: a search
    that does not hit the number exactly raises PROCESSING_ERROR and writes nothing).  The result gains
    `target` = dict(target_g_points, scaling, ng, status, tolerance_used[nband], trials) and the file the tool's extra variables.
    One process only, and neither cloud nor sequential_bands (PARAMETER_ERROR)."""
    import torch
    if cloud is not None and ssi is None:
        raise EcckdError(PARAMETER_ERROR, "Don't yet know how to sort cloud properties in the longwave")
    dev = ctx.device
    nband = len(band_bound1)
    ngas = len(gases)
    rank, world_size, tasks, mine, my_bands = _deal(ngas, nband, rank, world_size, group)
    target_mode = target_g_points is not None
    if target_mode:
        if world_size > 1:
            raise EcckdError(PARAMETER_ERROR, "target_g_points needs all gases in one process: a trial would need an all-reduce")
        if cloud is not None:
            raise EcckdError(PARAMETER_ERROR, "target_g_points cannot be combined with cloud")
        if sequential_bands:
            raise EcckdError(PARAMETER_ERROR, "target_g_points cannot be combined with sequential_bands")
        if int(target_g_points) < 1:
            raise EcckdError(PARAMETER_ERROR, "target_g_points = %d, must be at least 1" % int(target_g_points))
    prepared = []                  # target_g_points: (gas index, g, gas handle, sorting variable sorted, band albedo)
    tol = np.broadcast_to(np.asarray(heating_rate_tolerance, dtype=np.float64), (nband,))           # :762-771
    first_lw_gas = None
    planck_first = None            # the first gas's Planck matrix where this process does not prepare the first gas itself
    local = []                     # (gas index, band, result of the search)
    for gi in sorted(my_bands):
        spec = gases[gi]
        s = ncio.read_spectrum(spec["input"], iprofile)
        order = ncio.read_order(spec["reordering_input"])
        wn = s["wavenumber_cm_1"]
        bg = None
        for item in spec.get("background", []):                                                       # read_merged_spectrum (:891)
            b = ncio.read_spectrum(item["path"], iprofile)
            sp, _ = api.merge_scaling(b["pressure_hl"], item.get("scaling", -1.0), item.get("conc", -1.0),
                                      b["reference_surface_vmr"], b["vmr_fl"])
            bg = api.merge_spectrum(ctx, _to_device(b["optical_depth"], dev), sp, bg)
        iband = order["band_number"]
        idx = [np.nonzero(iband == b)[0] for b in range(nband)]
        g = dict(pressure_hl=s["pressure_hl"], temperature_hl=s["temperature_hl"], wn=torch.as_tensor(wn, device=dev),
                 dwn=torch.as_tensor(s["d_wavenumber_cm_1"], device=dev), rank=torch.as_tensor(order["rank"], device=dev),
                 od=_to_device(s["optical_depth"], dev), bg=bg, sorting_variable=torch.as_tensor(order["sorting_variable"], device=dev),
                 band_begin=[int(i[0]) if i.size else -1 for i in idx], band_end=[int(i[-1]) if i.size else -1 for i in idx],
                 min_g_points=np.broadcast_to(np.asarray(spec.get("min_g_points", 1)), (nband,)),       # per band, :733-754
                 max_g_points=np.broadcast_to(np.asarray(spec.get("max_g_points", 256)), (nband,)),
                 min_scaling=spec.get("min_scaling", 1.0), max_scaling=spec.get("max_scaling", 1.0))
        sw = reuse = None
        if ssi is None:
            # the reference evaluates the Planck function once, on the FIRST gas's reordered grid, and keeps using that
            # matrix for the later gases (find_g_points.cpp:529, :970-984): reproduced.  The process that prepares the first
            # gas keeps it alive; any other builds the same matrix from the first gas's ordering file and profile
            if gi > 0 and first_lw_gas is not None:
                reuse = first_lw_gas.view_ptr("planck_hl")[0]
            elif gi > 0:
                if planck_first is None:
                    s0 = ncio.read_spectrum(gases[0]["input"], iprofile, optical_depth=False)
                    o0 = ncio.read_order(gases[0]["reordering_input"])
                    planck_first = api.planck_hl_sorted(ctx, s0["temperature_hl"], torch.as_tensor(s0["wavenumber_cm_1"], device=dev),
                                                        torch.as_tensor(s0["d_wavenumber_cm_1"], device=dev),
                                                        torch.as_tensor(o0["rank"], device=dev))
                reuse = planck_first.data_ptr()
        else:
            b2 = np.asarray(band_bound2, dtype=np.float64)
            no_ray = b2 <= max_no_rayleigh_wavenumber
            wn_limit = b2[no_ray].max() if no_ray.any() else 0.0                                      # :761
            sw = dict(ssi=torch.as_tensor(np.asarray(ssi, dtype=np.float64), device=dev), cos_sza=cos_sza,
                      band_albedo=np.where(no_ray, reference_albedo, 0.0),                            # :756-760
                      albedo=torch.as_tensor(np.where(wn < wn_limit, reference_albedo, 0.0), device=dev))   # :921-923
        if target_mode:
            # prepared and kept resident; searched below, once every gas is prepared
            gas, sv_sorted, band_albedo = _prepare_gas(ctx, g, averaging_method, flux_weight, min_pressure, reuse, sw)
            prepared.append((gi, g, gas, sv_sorted, band_albedo))
            if ssi is None and gi == 0:
                first_lw_gas = gas
            continue
        gas, res = _search_gas(ctx, g, my_bands[gi], tol, tolerance_tolerance, max_iterations, averaging_method, flux_weight,
                               min_pressure, sequential_bands, reuse, sw)
        local += [(gi, b, r) for b, r in res]
        if ssi is None and gi == 0:
            first_lw_gas = gas
        else:
            gas.close()
    target = None
    if target_mode:
        reqs = [_band_requests(g, my_bands[gi], tol, band_albedo) for gi, g, _, _, band_albedo in prepared]
        try:
            found, info = api.find_g_gases_target([p[2] for p in prepared], reqs, nband * (1 - ngas), int(target_g_points),
                                                  target_resolution, target_max_trials, tolerance_tolerance, max_iterations)
            if target_exact and info["status"] != 0:
                raise EcckdError(PROCESSING_ERROR, "target_exact: no tolerance scaling gives %d g points (nearest: %d at scaling %.17g, "
                                 "search status %d)" % (int(target_g_points), info["ng"], info["scaling"], info["status"]))
            for (gi, g, gas, sv_sorted, _), band_res in zip(prepared, found):
                local += [(gi, b, r) for b, r in _finish_gas(gas, g, my_bands[gi], band_res, sv_sorted)]
        finally:
            for _, _, gas, _, _ in prepared:
                if gas is not first_lw_gas:
                    gas.close()
        # every gas has the same tolerances: those of the first
        target = dict(target_g_points=int(target_g_points), scaling=info["scaling"], ng=info["ng"], status=info["status"],
                      tolerance_used=info["tolerance_used"][0], trials=info["trials"])
    if first_lw_gas is not None:
        first_lw_gas.close()
    planck_first = None
    by_task, cost_sum, comp_sum = _collect(local, len(tasks), rank, world_size, group, dev)
    if rank != 0:
        return dict(rank=rank, tasks=mine, cost_sum=cost_sum, comp_cost_sum=comp_sum)
    # ---- what follows the gas loop (:1452-1660) ----
    per_gas = _per_gas_tables([spec["name"] for spec in gases], nband, by_task)
    gas_gp = []
    wn = None
    for spec, out in zip(gases, per_gas):
        order = ncio.read_order(spec["reordering_input"])
        wn = order["wavenumber"]
        gp = api.gas_g_point(ctx, torch.as_tensor(order["rank"], device=dev), out["rank1"], out["rank2"])
        out["g_point"] = gp.cpu().numpy()
        gas_gp.append(gp)
    if cloud is not None:
        out, gp = cloud_g_points(ctx, cloud, ssi, nwav=len(wn), nband=nband)
        out["g_point"] = gp.cpu().numpy()
        per_gas.insert(0, out)
        gas_gp.insert(0, gp)
    ng, band_number, g_min, g_max = api.overlap_g_points([g["n_g_points"] for g in per_gas],
                                                         [np.asarray(g["sorting_variable"]) for g in per_gas])
    g_point, n_unassigned = api.merge_g_points(ctx, gas_gp, g_min, g_max)
    for k, g in enumerate(per_gas):
        g["g_min"], g["g_max"] = g_min[k], g_max[k]
    result = dict(ng=ng, band_number=band_number, g_point=g_point.cpu().numpy(), n_unassigned=n_unassigned, gases=per_gas,
                  wavenumber=wn, cost_sum=cost_sum, comp_cost_sum=comp_sum, rank=0, tasks=mine)
    if target is not None:
        result["target"] = target
    if output_path is not None:
        ncio.write_g_points(output_path, band_bound1, band_bound2, band_number, per_gas, wn, result["g_point"], target=target)
    return result


def find_g_points_resident(ctx, names, load_gas, nband, heating_rate_tolerance, first_gas_order=None, averaging_method="transmission",
                           flux_weight=0.02, min_pressure=0.0, tolerance_tolerance=0.02, max_iterations=60,
                           sequential_bands=False, rank=None, world_size=None, group=None, merged_map=True, sw=None,
                           gases_side_by_side=1):
    """find_g_points on spectra that are already resident in HBM (bench.py, the full-size tests): the same dealing of the
    (gas, band) tasks, the same per-gas work (_search_gas) and the same collection as find_g_points, with `load_gas(gi)`
    handing over the device tensors of gas gi (the dict _search_gas takes; the call may do the gas's reorder_spectrum step,
    K1 + K3, itself) instead of reading files.  Longwave unless `sw` is given: dict(ssi, albedo: device tensors,
    band_albedo[nband], cos_sza) as _search_gas takes it (no shared Planck matrix then; first_gas_order is only asked for the
    number of wavenumbers by a process without tasks).

    first_gas_order: callable -> dict(temperature_hl, wn, dwn, rank) of the FIRST gas for a process that searches none of
    its bands (what the file driver reads from the first gas's ordering file), for the shared Planck matrix.
    merged_map: every gas's per-wavenumber g points travel to rank 0 (one reduce per gas; each wavenumber is set by exactly
    one process), which forms the merged g-point map (:1459-1475).
    gases_side_by_side: 1 = gas after gas as the reference's loop (:655): load, prepare, search, release; otherwise every gas
    of this process is loaded and prepared first (all resident: ~9.5 GB per gas at 7.2e6 points), then ALL their band searches
    run side by side (ecckd_find_g_gases: one host thread and HIP stream per gas; n > 1: at most n gases at a time, 0: what the
    host has cores for) - same g points, same errors, the gases' latency-bound batches in each other's shadow.
    -> rank 0: dict(ng, band_number, gases, g_point (device), n_unassigned, cost_sum, comp_cost_sum, points);
       others: dict(cost_sum, comp_cost_sum, points).  `points`: wavenumber points this process worked through: one pass over its bands (reorder, preparation) + the points
    its searches swept on the device (an interval asked for twice is swept once: the memo of interval errors)."""
    import torch
    dev = ctx.device
    ngas = len(names)
    rank, world_size, tasks, mine, my_bands = _deal(ngas, nband, rank, world_size, group)
    tol = np.broadcast_to(np.asarray(heating_rate_tolerance, dtype=np.float64), (nband,))
    first_lw_gas = None
    planck_first = None
    import time
    local, maps = [], {}
    points = 0.0
    nwav = None
    phase = {"reorder": 0.0, "preparation": 0.0, "search": 0.0, "medians": 0.0, "maps": 0.0, "collect": 0.0}
    side_by_side = gases_side_by_side != 1 and len(my_bands) > 1
    prepared = {}
    if side_by_side:
        # every gas of this process is loaded and prepared; its searches start as soon as it is (GasSearchJob.add returns at once)
        # and run while the next gas is merged, reordered and prepared on the context's stream
        job = api.GasSearchJob(tolerance_tolerance, max_iterations, max_concurrent=gases_side_by_side)
        ts = None
        order = sorted(my_bands)
        for gi in order:
            tl = time.perf_counter()
            g = load_gas(gi)
            ctx.synchronize()
            phase["reorder"] += time.perf_counter() - tl
            reuse = None
            if sw is not None:
                pass
            elif gi > 0 and first_lw_gas is not None:
                reuse = first_lw_gas.view_ptr("planck_hl")[0]
            elif gi > 0:
                if planck_first is None:
                    o0 = first_gas_order()
                    planck_first = api.planck_hl_sorted(ctx, o0["temperature_hl"], o0["wn"], o0["dwn"], o0["rank"])
                reuse = planck_first.data_ptr()
            gas, sv_sorted, band_albedo = _prepare_gas(ctx, g, averaging_method, flux_weight, min_pressure, reuse, sw)
            for k in ("od", "bg", "bg_sources"):  # the spectra are in the gas's rows now
                g.pop(k, None)
            req = _band_requests(g, my_bands[gi], tol, band_albedo)
            prepared[gi] = (g, gas, sv_sorted)
            if gi == 0 and sw is None:
                first_lw_gas = gas
            ts = ts or time.perf_counter()
            job.add(gas, req["ibegin"], req["iend"], req["heating_rate_tolerance"], req["options"])
        tw = time.perf_counter()
        all_res = job.wait()
        phase["search"] += time.perf_counter() - tw           # what is left of the searches when the last gas is prepared
        phase["search_window"] = phase.get("search_window", 0.0) + time.perf_counter() - ts
        for gi, band_res in zip(order, all_res):
            g, gas, sv_sorted = prepared[gi]
            prepared[gi] = (g, gas, _finish_gas(gas, g, my_bands[gi], band_res, sv_sorted))
    for gi in sorted(my_bands):
        if side_by_side:
            g, gas, res = prepared.pop(gi)
            nwav = g["rank"].numel()
        else:
            tl = time.perf_counter()
            g = load_gas(gi)
            ctx.synchronize()
            phase["reorder"] += time.perf_counter() - tl
            nwav = g["rank"].numel()
            reuse = None
            if sw is not None:
                pass
            elif gi > 0 and first_lw_gas is not None:
                reuse = first_lw_gas.view_ptr("planck_hl")[0]
            elif gi > 0:
                if planck_first is None:
                    o0 = first_gas_order()
                    planck_first = api.planck_hl_sorted(ctx, o0["temperature_hl"], o0["wn"], o0["dwn"], o0["rank"])
                reuse = planck_first.data_ptr()
            gas, res = _search_gas(ctx, g, my_bands[gi], tol, tolerance_tolerance, max_iterations, averaging_method, flux_weight,
                                   min_pressure, sequential_bands, reuse, sw)
        for b, r in res:
            r["index_range"] = (int(g["band_begin"][b]), int(g["band_end"][b]))
            points += g["band_end"][b] - g["band_begin"][b] + 1            # the reorder / preparation pass over the band
        points += gas.eval_stats()["points_evaluated"]                       # what the searches swept on the device
        local += [(gi, b, r) for b, r in res]
        for k in ("preparation", "search", "medians"):
            phase[k] += g["timing"].get(k, 0.0)
        tm = time.perf_counter()
        if merged_map:
            # this process's bands of the gas: (band << 16) + g point of every wavenumber counted from the band's first (-1
            # elsewhere).  One launch over the spectrum with the bands' rank ranges one after the other (a band's ranks lie in its
            # own index range, so no other band's wavenumbers fall into them), then from that running count to band and count
            # within the band - what the root can renumber once it knows every band's number of g points.
            if res:
                r1 = np.concatenate([np.asarray(r["rank1"], dtype=np.int64) for _, r in res])
                r2 = np.concatenate([np.asarray(r["rank2"], dtype=np.int64) for _, r in res])
                assert nband < 32768 and all(len(r["rank1"]) < 65536 for _, r in res)
                within = np.concatenate([(b << 16) + np.arange(len(r["rank1"]), dtype=np.int32) for b, r in res]).astype(np.int32)
                gp = api.gas_g_point(ctx, g["rank"], r1, r2)
                tbl = torch.as_tensor(within, device=dev)
                gp = torch.where(gp >= 0, tbl[gp.clamp(min=0).long()], gp)
            else:
                gp = torch.full((nwav,), -1, dtype=torch.int32, device=dev)
            maps[gi] = gp
        if gi == 0 and sw is None:
            first_lw_gas = gas
        else:
            gas.close()
        phase["maps"] += time.perf_counter() - tm
    if first_lw_gas is not None:
        first_lw_gas.close()
    planck_first = None
    tc = time.perf_counter()
    by_task, cost_sum, comp_sum = _collect(local, len(tasks), rank, world_size, group, dev)
    gas_gp = []
    if merged_map:
        if nwav is None:
            nwav = first_gas_order()["rank"].numel()
        for gi in range(ngas):
            gp = maps.get(gi)
            if gp is None:
                gp = torch.full((nwav,), -1, dtype=torch.int32, device=dev)
            gas_gp.append(_max_to_root(gp, world_size, group))
    if rank != 0:
        phase["collect"] = time.perf_counter() - tc
        return dict(rank=rank, tasks=mine, cost_sum=cost_sum, comp_cost_sum=comp_sum, points=points, phase_seconds=phase)
    per_gas = _per_gas_tables(names, nband, by_task)
    ng, band_number, g_min, g_max = api.overlap_g_points([g["n_g_points"] for g in per_gas],
                                                         [np.asarray(g["sorting_variable"]) for g in per_gas])
    result = dict(ng=ng, band_number=band_number, gases=per_gas, cost_sum=cost_sum, comp_cost_sum=comp_sum, rank=0, tasks=mine,
                  points=points, phase_seconds=phase)
    for k, g in enumerate(per_gas):
        g["g_min"], g["g_max"] = g_min[k], g_max[k]
    if merged_map:
        # the gathered maps hold (band << 16) + the g point counted from the band's first: add the number of g points of the gas's
        # earlier bands (SingleGasData::store_g_points numbers them through the bands, single_gas_data.h:56-62)
        for gi, (gp, out) in enumerate(zip(gas_gp, per_gas)):
            first = torch.as_tensor(np.concatenate([[0], np.cumsum(out["n_g_points"])[:-1]]).astype(np.int32), device=gp.device)
            renumbered = first[(gp >> 16).clamp(min=0).long()] + (gp & 0xffff)
            gas_gp[gi] = torch.where(gp >= 0, renumbered, gp)
        result["g_point"], result["n_unassigned"] = api.merge_g_points(ctx, gas_gp, g_min, g_max)
        result["gas_g_point"] = gas_gp
    phase["collect"] = time.perf_counter() - tc
    return result


def _max_to_root(t, world_size, group=None):
    """Element-wise maximum over the processes on rank 0 (one reduce; gloo works on a host copy)."""
    if world_size == 1:
        return t
    import torch.distributed as dist
    if _is_nccl(group):
        dist.reduce(t, dst=0, op=dist.ReduceOp.MAX, group=group)
        return t
    h = t.cpu()
    dist.reduce(h, dst=0, op=dist.ReduceOp.MAX, group=group)
    return h.to(t.device)


def _is_nccl(group=None):
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_backend(group) == "nccl"


def _read_merged_spectrum(ctx, inputs, scaling, conc, icol):
    """read_merged_spectrum.cpp:20-185 as cli/tool.hpp::read_merged_spectrum does it (without a concentration file): every
    file's optical depths to the device as stored, scaling rules on the host, sum on the device.  A single unscaled input
    stays as stored (FLOAT).  -> (first spectrum dict, molecules, device optical depths, vmr rows)"""
    import torch
    first, molecules, merged, vmr = None, "", None, []
    for ibg, path in enumerate(inputs):
        s = ncio.read_spectrum(path, icol)
        sc = scaling[ibg] if scaling is not None and ibg < len(scaling) else -1.0
        cc = conc[ibg] if conc is not None and ibg < len(conc) else -1.0
        if ibg == 0:
            first, molecules = s, s["molecule"] or ""
        else:
            molecules += " " + (s["molecule"] or "")
        sp, vrow = api.merge_scaling(first["pressure_hl"], sc, cc, s["reference_surface_vmr"], s["vmr_fl"])
        vmr.append(vrow)
        od = _to_device(s["optical_depth"], ctx.device)
        if len(inputs) == 1 and np.all(sp == 1.0):
            merged = od
        else:
            merged = api.merge_spectrum(ctx, od, sp, merged)
    ctx.synchronize()
    return first, molecules, merged, np.array(vmr)


MAX_SCENARIO_INPUTS = 16


def _check_scenarios(scenarios, inputs, read_files, **beside):
    """The checks of the tools' scenarios= key (cli/spectra.hpp), before anything touches a device: `scenarios` a list of
    dict(name=, output=, scaling=[...] or None, conc=[...] or None) with one scaling / conc per file of `inputs` (None or a
    negative number: as the file holds the gas); `read_files`: {key: file} of whatever else the run reads; `beside`: the
    arguments that come from the table.  -> the entries as (name, output, scaling, conc); ValueError otherwise."""
    for key, value in beside.items():
        if value is not None:
            raise ValueError(f'"{key}" cannot be combined with "scenarios" (outputs and scalings come from the table)')
    inputs = [str(p) for p in inputs]
    if not inputs:
        raise ValueError("Unable to read input file names in input")
    if len(inputs) > MAX_SCENARIO_INPUTS:
        raise ValueError(f'"scenarios": {len(inputs)} input files, {MAX_SCENARIO_INPUTS} at most')
    scenarios = list(scenarios)
    if not scenarios:
        raise ValueError("Scenario table is empty")
    table, outputs = [], set()
    for line, entry in enumerate(scenarios, 1):
        unknown = set(entry) - {"name", "output", "scaling", "conc"}
        if "const" in unknown:
            raise ValueError(f"scenario {line}: const=C is not a scaling of lw_spectra / sw_spectra (scaling or conc)")
        if unknown or "name" not in entry:
            raise ValueError(f"scenario {line}: unknown scaling spec {sorted(unknown)} (name, output, scaling, conc)")
        row = [entry["name"], entry.get("output")]
        for key in ("scaling", "conc"):
            v = entry.get(key)
            if v is not None:
                v = [-1.0 if x is None else float(x) for x in v]
                if len(v) != len(inputs):
                    raise ValueError(f"scenario {line}: {len(v)} {key} value(s) for {len(inputs)} spectrum file(s) (one per file)")
            row.append(v)
        out = row[1]
        if out is not None:
            out = str(out)
            if out in outputs:
                raise ValueError(f'scenario {line}: duplicate output file "{out}"')
            outputs.add(out)
            for key, f in [("input", p) for p in inputs] + [(k, str(f)) for k, f in read_files.items() if f is not None]:
                if _same_file(out, f):
                    raise ValueError(f'scenario {line}: the output "{out}" is the {key} file of this run')
        table.append(tuple(row))
    return table


def _same_file(a, b):
    import os
    return a == b or (os.path.exists(a) and os.path.exists(b) and os.path.realpath(a) == os.path.realpath(b))


def _read_column_gases(ctx, inputs, icol):
    """One column of every gas file, read once: -> (first spectrum dict, molecules, [(device optical depths as stored,
    reference_surface_vmr, vmr_fl)])"""
    first, molecules, gases = None, "", []
    for ibg, path in enumerate(inputs):
        s = ncio.read_spectrum(path, icol)
        if ibg == 0:
            first, molecules = s, s["molecule"] or ""
        else:
            molecules += " " + (s["molecule"] or "")
        gases.append((_to_device(s["optical_depth"], ctx.device), s["reference_surface_vmr"], s["vmr_fl"]))
    return first, molecules, gases


def _merge_scenario(ctx, first, gases, scaling, conc, merged):
    """A scenario of a column read by _read_column_gases: the scaling rules on the host, all gases merged in one pass into
    `merged` (allocated when None; every scenario fills it again).  A single unscaled input stays as stored.
    -> (device optical depths, vmr rows, merged)"""
    profiles, vmr = [], []
    for ibg, (od, ref, vmr_fl) in enumerate(gases):
        sp, vrow = api.merge_scaling(first["pressure_hl"], -1.0 if scaling is None else scaling[ibg], -1.0 if conc is None else conc[ibg],
                                     ref, vmr_fl)
        profiles.append(sp)
        vmr.append(vrow)
    if len(gases) == 1 and np.all(profiles[0] == 1.0):
        return gases[0][0], np.array(vmr), merged
    merged = api.merge_scenario(ctx, [g[0] for g in gases], np.array(profiles), merged=merged)
    ctx.synchronize()
    return merged, np.array(vmr), merged


def merge_spectra(ctx, inputs, output_path=None, scaling=None, conc=None, config_str="", history=None):
    """merge_spectra.cpp:27-170: the spectra of several gases merged column by column, as bin/merge_spectra does it.
    -> dict(pressure_hl, temperature_hl (ncol, nlay+1), wavenumber, optical_depth (ncol, nlay, nwav) as the file's FLOATs,
    molecules); written to output_path when given."""
    out = {"pressure_hl": [], "temperature_hl": [], "optical_depth": []}
    icol, ncol = 0, 1
    while icol < ncol:
        first, molecules, merged, _ = _read_merged_spectrum(ctx, inputs, scaling, conc, icol)
        ncol = first["ncol"]
        out["pressure_hl"].append(first["pressure_hl"])
        out["temperature_hl"].append(first["temperature_hl"])
        out["optical_depth"].append(merged.cpu().numpy().astype(np.float32))
        out["wavenumber"], out["molecules"] = first["wavenumber_cm_1"], molecules
        icol += 1
    for k in ("pressure_hl", "temperature_hl", "optical_depth"):
        out[k] = np.stack(out[k])
    if output_path is not None:
        ncio.write_merged_spectra(output_path, out, config_str=config_str, history=history)
    return out


def lw_spectra(ctx, inputs, output_path=None, scaling=None, conc=None, g_point=None, iprofile=None, config_str="", history=None,
               nangle=0, scenarios=None):
    """lw_spectra.cpp:31-275 as bin/lw_spectra does it: per column the merged spectrum, then either the spectral fluxes
    (ecckd_lbl_spectral_fluxes_lw) or, with g_point (one value per wavenumber, -1 = none), the fluxes per g point
    (ecckd_lbl_gpoint_fluxes_lw) and the optical depth averaged by transmission with the Planck weight at the pressure-weighted
    full-level temperature (ecckd_average_to_gpoints, reference_surface_vmr = 0).  nangle (the tool's key): 0 the two-stream
    fluxes, N > 0 those of N Gauss-Legendre zenith angles per hemisphere.  Arrays are returned in double as the library
    gives them (the tool's file holds their FLOAT casts): dict of (nrec, ...) arrays; written to output_path when given.
    scenarios (the tool's scenarios= key): a list of dict(name=, output=, scaling=[...] or None, conc=[...] or None) in place of
    output_path, scaling and conc: every gas file is read once per column, every scenario merged from that read in one pass
    (api.merge_scenario) -> the list of those dicts, one per scenario in table order, each written where its `output` is set."""
    import torch
    table = None
    if scenarios is not None:
        table = _check_scenarios(scenarios, inputs, {}, output_path=output_path, scaling=scaling, conc=conc)
    names = ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw",
             "spectral_flux_up_lw")
    outs = [{k: [] for k in names} for _ in (table or [None])]
    have_g = g_point is not None
    ng = int(np.max(g_point)) + 1 if have_g else -1
    icol = iprofile if iprofile is not None else 0
    ncol, gm, d_wn, d_dwn, shared = 10000, None, None, None, None
    while icol < ncol:
        if table is not None:
            first, molecules, gases = _read_column_gases(ctx, inputs, icol)        # the one read of this column
        for k, out in enumerate(outs):
            if table is None:
                first, molecules, od, vmr = _read_merged_spectrum(ctx, inputs, scaling, conc, icol)
            else:
                od, vmr, shared = _merge_scenario(ctx, first, gases, table[k][2], table[k][3], shared)
            ncol = first["ncol"]
            p, t = first["pressure_hl"], first["temperature_hl"]
            if d_wn is None:
                d_wn = torch.as_tensor(first["wavenumber_cm_1"], device=ctx.device)
                d_dwn = torch.as_tensor(first["d_wavenumber_cm_1"], device=ctx.device)
                if have_g:
                    gm = api.GPointMap(ctx, torch.as_tensor(np.ascontiguousarray(g_point, dtype=np.int32), device=ctx.device), ng, d_wn, d_dwn)
            out["wavenumber"], out["molecules"] = first["wavenumber_cm_1"], molecules.replace(",", " ")
            out["pressure_hl"].append(p)
            out["temperature_hl"].append(t)
            out["vmr_fl"].append(vmr)
            if not have_g:
                sdn, sup, bdn, bup = api.lbl_spectral_fluxes_lw(ctx, t, d_wn, d_dwn, od, nangle=nangle)
                out["optical_depth"].append(od.cpu().numpy().astype(np.float64))
                out["spectral_flux_dn_lw"].append(sdn.cpu().numpy().astype(np.float64))
                out["spectral_flux_up_lw"].append(sup.cpu().numpy().astype(np.float64))
            else:
                dn, up, bdn, bup = gm.lbl_fluxes_lw(t, od, nangle=nangle)
                p_fl = 0.5 * (p[:-1] + p[1:])
                t_fl = 0.5 * (t[:-1] * p[:-1] + t[1:] * p[1:]) / p_fl                              # :242-244
                od_g, _, _ = gm.average_optical_depth(p, od, "transmission", 0.0, temperature_fl=t_fl)
                out["optical_depth"].append(od_g)
                out["spectral_flux_dn_lw"].append(dn)
                out["spectral_flux_up_lw"].append(up)
            out["flux_dn_lw"].append(bdn)
            out["flux_up_lw"].append(bup)
        if iprofile is not None:
            break
        icol += 1
    if gm is not None:
        gm.close()
    for k, out in enumerate(outs):
        for name in names:
            out[name] = np.stack(out[name])
        out["ng"] = ng
        out["nangle"] = int(nangle)
        path = output_path
        if table is not None:
            out["scenario"], path = table[k][0], table[k][1]
        if path is not None:
            ncio.write_lw_spectra(path, out, config_str=config_str, history=history)
    return outs if table is not None else outs[0]


def sw_spectra(ctx, inputs, ssi, output_path=None, scaling=None, conc=None, g_point=None, iprofile=None, cos_sza=(0.5,),
               surface_albedo=0.15, config_str="", history=None, rayleigh=None, scenarios=None):
    """bin/sw_spectra as the tool does it: per column the merged spectrum, then either the spectral fluxes one angle at a time
    (ecckd_lbl_spectral_fluxes_sw) or, with g_point (one value per wavenumber, -1 = none), the fluxes per g point for all
    angles in one call (ecckd_lbl_gpoint_fluxes_sw) and the optical depth averaged by transmission with the `ssi` weight
    (ecckd_average_to_gpoints, reference_surface_vmr = 0).  `ssi`: solar spectral irradiance per wavenumber (host array).
    `rayleigh`: the path of a spectrum file whose optical_depth scatters (the tool's key): the fluxes are those of the two-stream
    transfer (ecckd_lbl_spectral_fluxes_sw_rayleigh / ecckd_lbl_gpoint_fluxes_sw_rayleigh), flux_dn_sw and spectral_flux_dn_sw
    (direct plus diffuse) are returned too and, with g_point, rayleigh_optical_depth: that spectrum averaged like optical_depth.
    Arrays are returned in double as the library gives them (the tool's file holds their FLOAT casts): dict of (nrec, ...)
    arrays; written to output_path when given.
    scenarios: as in lw_spectra - the gas files are read once per column, the spectrum of `rayleigh` too and never scaled ->
    the list of the result dicts, one per scenario in table order."""
    import torch
    table = None
    if scenarios is not None:
        table = _check_scenarios(scenarios, inputs, {"rayleigh": rayleigh}, output_path=output_path, scaling=scaling, conc=conc)
    names = ["pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_direct_sw", "flux_up_sw", "optical_depth",
             "spectral_flux_dn_direct_sw", "spectral_flux_up_sw"]
    have_g = g_point is not None
    if rayleigh is not None:
        names += ["flux_dn_sw", "spectral_flux_dn_sw"] + (["rayleigh_optical_depth"] if have_g else [])
    outs = [{k: [] for k in names} for _ in (table or [None])]
    mu0 = np.atleast_1d(np.asarray(cos_sza, dtype=np.float64))
    if not (1 <= mu0.size <= 8) or np.any(~((mu0 > 0.0) & (mu0 <= 1.0))):
        raise EcckdError(PARAMETER_ERROR, "cos_sza must hold 1 to 8 numbers in (0, 1]")
    ng = int(np.max(g_point)) + 1 if have_g else -1
    if have_g and ng < 1:
        raise EcckdError(PARAMETER_ERROR, "g_point assigns no wavenumber to a g point")
    icol = iprofile if iprofile is not None else 0
    ncol, gm, d_ssi, d_albedo, shared, solar = 10000, None, None, None, None, None
    while icol < ncol:
        if table is not None:
            first, molecules, gases = _read_column_gases(ctx, inputs, icol)        # the one read of this column
        ray = None
        for k, out in enumerate(outs):
            if table is None:
                first, molecules, od, vmr = _read_merged_spectrum(ctx, inputs, scaling, conc, icol)
            else:
                od, vmr, shared = _merge_scenario(ctx, first, gases, table[k][2], table[k][3], shared)
            ncol = first["ncol"]
            p, t = first["pressure_hl"], first["temperature_hl"]
            if d_ssi is None:
                nwav = first["wavenumber_cm_1"].size
                if np.size(ssi) != nwav or (have_g and np.size(g_point) != nwav):
                    raise EcckdError(PARAMETER_ERROR, "ssi / g_point do not have one value per wavenumber")
                d_ssi = torch.as_tensor(np.ascontiguousarray(ssi, dtype=np.float64), device=ctx.device)
                d_albedo = torch.full((nwav,), float(surface_albedo), dtype=torch.float64, device=ctx.device)
                if have_g:
                    d_wn = torch.as_tensor(first["wavenumber_cm_1"], device=ctx.device)
                    d_dwn = torch.as_tensor(first["d_wavenumber_cm_1"], device=ctx.device)
                    gm = api.GPointMap(ctx, torch.as_tensor(np.ascontiguousarray(g_point, dtype=np.int32), device=ctx.device), ng, d_wn, d_dwn)
                    solar = gm.sum_rows(d_ssi[None, :])[0]
            if have_g:
                out["solar_irradiance"] = solar
            out["wavenumber"], out["molecules"] = first["wavenumber_cm_1"], molecules.replace(",", " ")
            if rayleigh is not None and ray is None:     # the spectrum that scatters: this column of it, unscaled, as it is stored
                r = ncio.read_spectrum(rayleigh, icol)
                if not np.array_equal(r["wavenumber_cm_1"], first["wavenumber_cm_1"]) or r["pressure_hl"].size != p.size or r["ncol"] != ncol:
                    raise EcckdError(PARAMETER_ERROR, "the Rayleigh spectrum does not have the merged spectrum's wavenumbers, levels and columns")
                ray = _to_device(r["optical_depth"], ctx.device)
            out["pressure_hl"].append(p)
            if t is not None:
                out["temperature_hl"].append(t)
            out["vmr_fl"].append(vmr)
            if not have_g:
                sdn, sup, stot, bdn, bup, btot = [], [], [], [], [], []
                for mu in mu0:                                                                     # one angle at a time, as the tool
                    if ray is not None:
                        a, e, b, c, f, d = api.lbl_spectral_fluxes_sw_rayleigh(ctx, mu, d_ssi, od, ray, d_albedo)
                        stot.append(e[0].cpu().numpy().astype(np.float64))
                        btot.append(f[0])
                    else:
                        a, b, c, d = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, od, d_albedo)
                    sdn.append(a[0].cpu().numpy().astype(np.float64))
                    sup.append(b[0].cpu().numpy().astype(np.float64))
                    bdn.append(c[0])
                    bup.append(d[0])
                bdn, bup = np.stack(bdn), np.stack(bup)
                if ray is not None:
                    out["spectral_flux_dn_sw"].append(np.stack(stot))
                    out["flux_dn_sw"].append(np.stack(btot))
                out["optical_depth"].append(od.cpu().numpy().astype(np.float64))
                out["spectral_flux_dn_direct_sw"].append(np.stack(sdn))
                out["spectral_flux_up_sw"].append(np.stack(sup))
            else:
                if ray is not None:
                    dn, tot, up, bdn, btot, bup = gm.lbl_fluxes_sw_rayleigh(mu0, d_ssi, od, ray, d_albedo)
                    out["spectral_flux_dn_sw"].append(tot)
                    out["flux_dn_sw"].append(btot)
                    out["rayleigh_optical_depth"].append(gm.average_optical_depth(p, ray, "transmission", 0.0, ssi=d_ssi)[0])
                else:
                    dn, up, bdn, bup = gm.lbl_fluxes_sw(mu0, d_ssi, od, d_albedo)
                od_g, _, _ = gm.average_optical_depth(p, od, "transmission", 0.0, ssi=d_ssi)
                out["optical_depth"].append(od_g)
                out["spectral_flux_dn_direct_sw"].append(dn)
                out["spectral_flux_up_sw"].append(up)
            out["flux_dn_direct_sw"].append(bdn)
            out["flux_up_sw"].append(bup)
        if iprofile is not None:
            break
        icol += 1
    if gm is not None:
        gm.close()
    for k, out in enumerate(outs):
        kept = list(names)
        if not out["temperature_hl"]:
            del out["temperature_hl"]
            kept.remove("temperature_hl")
        for name in kept:
            out[name] = np.stack(out[name])
        out["ng"], out["mu0"] = ng, mu0
        if rayleigh is not None:
            out["rayleigh"] = True                      # write_sw_spectra: the variables and the attribute the key adds
        path = output_path
        if table is not None:
            out["scenario"], path = table[k][0], table[k][1]
        if path is not None:
            ncio.write_sw_spectra(path, out, config_str=config_str, history=history)
    return outs if table is not None else outs[0]
