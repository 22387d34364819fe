"""The reference's file pipeline: em_sample (model -> initial.txt / transition.txt) and sample2track
(those files -> 1 Hz dead-reckoning tracks as CSV), RUN_1_emsample.m / RUN_2_sample2track.m.

Same names, arguments and file formats as code/matlab/em_sample.m and code/matlab/sample2track.m.
Sampling and the track integration run on the GPU (libemgpu: emgpu_sample_dbn_host,
emgpu_sample2track_host); parsing and formatting are host-side Python, as they are host-side MATLAB
in the reference -- em_sample(text="device") formats its rows on the GPU too (emgpu_sample_text_host) and
writes the same bytes, and sample2track(text="device") parses both files, integrates the tracks and formats the CSV rows on the GPU
(emgpu_parse_table_host, emgpu_tracks_text_host) and writes the same files.  A device-resident consumer that skips the text files exists as
native.sample2track_device (it reads the sampler's dense trace in place).
"""
import os
import re
import time
import types

import numpy as np

from . import native
from .em_io import em_read
from .functions import _model_of, _take, bn_dirichlet_prior

FT_PER_NM = 1852.0 / 0.3048          # unitsratio('ft', 'nm')


# what the last em_sample(text="device") spent where: library calls, their phases (emgpu_host_stats, summed over the calls), file writes
last_text_stats = {}
# what the last sample2track(text="device") spent where: file reads, the library call and its phases (upload, the three kernel groups, download,
# host work), file writes; bytes, rows, hard tokens, host-formatted tracks
last_track_stats = {}


def _g(x):
    """fprintf('%g', x): C and Python agree, except for the spelling of non-finite values."""
    x = float(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    return "%g" % x


def em_sample(parameters_filename, initial_output_filename=None, transition_output_filename=None, num_initial_samples=100,
              num_transition_samples=60, start=None, isOverwriteZeroBoundaries=False, idxZeroBoundaries=(1, 2, 3),
              rng_seed=42, prior=0, ctx=None, text="host", return_arrays=True, id_first=1, text_batch=None, start_grid=None):
    """em_sample(parameters_filename, 'initial_output_filename', ..., 'num_initial_samples', 100,
    'num_transition_samples', 60, 'start', {}, 'rng_seed', 42)  (em_sample.m:1-104).

    Writes `id <labels_initial>` rows (dediscretised initial sample, %g) and `initial_id t <dynamic labels>`
    rows (the dense trace of the dynamic variables at t = 0 .. num_transition_samples-1).
    `prior`: em_sample.m:52 assigns the string 'constant', which bn_dirichlet_prior.m:28 rejects
    (prior:notdbe), so the reference as shipped stops there; the constant prior 0 is what its
    documentation describes and is the default here.  Returns (initial [n, n_initial], trace [n, T, n_dyn]).

    text: "host" formats every row in Python ("%g" per value); "device" writes the same two files from rows formatted on the GPU
    (native.sample_text_host), in batches of text_batch trajectories (default: as many as keep the pinned text buffers near 256 MiB, by
    native.text_bound), so host memory stays bounded whatever num_initial_samples is.  Device writer only: return_arrays=False returns
    (None, None) and keeps no array of the run; id_first is the id of the first trajectory (a run continued from an earlier file).

    start_grid: [num_initial_samples, n_initial] preset bins by variable id, one row per trajectory (0 / None = unset: `start`, else the
    variable is drawn): the strata of a loop over `start` values in one pair of files, under either writer.  The sampler is the +start instance
    of the kernel the model runs on without a grid (k_uncor_fast_idx, or k_dbn_step2 for cor_v1 and the other models outside the fast branch)."""
    if text not in ("host", "device"):
        raise ValueError("em_sample: text must be 'host' or 'device', not %r" % (text,))
    if text == "host" and (not return_arrays or int(id_first) != 1 or text_batch is not None):
        raise ValueError("em_sample: return_arrays=False, id_first and text_batch belong to text='device'")
    out_dir = os.path.join(os.environ.get("AEM_DIR_BAYES", "."), "output")
    initial_output_filename = initial_output_filename or os.path.join(out_dir, "initial.txt")
    transition_output_filename = transition_output_filename or os.path.join(out_dir, "transition.txt")
    parms = em_read(parameters_filename, isOverwriteZeroBoundaries=isOverwriteZeroBoundaries, idxZeroBoundaries=list(idxZeroBoundaries))
    di = bn_dirichlet_prior(parms["N_initial"], prior)
    dt = bn_dirichlet_prior(parms["N_transition"], prior)
    m = _model_of(parms, di, dt, start)
    n, T = int(num_initial_samples), int(num_transition_samples)
    grid = None
    if start_grid is not None:
        grid = np.array([[0 if (v is None or (isinstance(v, float) and np.isnan(v))) else int(v) for v in row] for row in start_grid], dtype=np.int32)
        if grid.shape != (n, m.n_initial):
            raise ValueError("em_sample: start_grid must have num_initial_samples rows of n_initial entries")
        native.start_grid_log_weight(m, grid)   # a bad row is reported with its number, before a file is touched
    seed, first = _take(rng_seed, n)
    tm = np.asarray(parms["temporal_map"]).reshape(-1, 2)
    header_initial = "id " + "".join("%s " % s for s in parms["labels_initial"]) + "\n"                                         # :64-68
    header_transition = "initial_id t " + "".join("%s " % parms["labels_transition"][int(r[1]) - 1] for r in tm) + "\n"       # :71-75
    for f in (initial_output_filename, transition_output_filename):
        if os.path.dirname(f):
            os.makedirs(os.path.dirname(f), exist_ok=True)
    if text == "device":
        return _em_sample_device_text(ctx or native.default_context(), m, n, T, seed, first, initial_output_filename, transition_output_filename,
                                      header_initial, header_transition, return_arrays, int(id_first), text_batch, grid)
    # dbn_hierarchical_sample + events2samples (em_sample.m:78-82): no rejection test, dense trace
    res = native.sample_dbn_host(ctx or native.default_context(), m, n, T, seed, first_index=first, want_dense=True,
                                 max_attempts=1, start=grid)
    initial = res["init_val"].astype(np.float64)
    trace = res["dyn_val"].astype(np.float64)
    with open(initial_output_filename, "w", encoding="utf-8", newline="\n") as f:
        f.write(header_initial)
        for i in range(n):
            f.write("%d " % (i + 1) + " ".join(_g(v) for v in initial[i]) + "\n")                # :85-88
    with open(transition_output_filename, "w", encoding="utf-8", newline="\n") as f:
        f.write(header_transition)
        rows = []
        for i in range(n):
            for j in range(T):
                rows.append("%s %s " % (_g(i + 1), _g(j)) + " ".join(_g(v) for v in trace[i, j]) + "\n")        # :91-96
        f.write("".join(rows))
    return initial, trace


def _em_sample_device_text(ctx, m, n, T, seed, first, initial_filename, transition_filename, header_initial, header_transition, return_arrays,
                           id_first, text_batch, grid=None):
    """em_sample's files from rows formatted on the device: batch after batch of trajectories through native.sample_text_host into one pair of
    pinned buffers, each batch's bytes appended to the files.  last_text_stats says where the time went."""
    st = {"calls": 0, "batch": 0, "library_ms": 0.0, "kernel_ms": 0.0, "d2h_ms": 0.0, "scatter_ms": 0.0, "write_ms": 0.0, "bytes": 0}
    per_i, per_t = native.text_bound(m, 1, T)
    batch = int(text_batch) if text_batch is not None else max(1024, (256 << 20) // max(per_t, per_i))
    batch = max(1, min(batch, max(n, 1)))
    buffers = (ctx.pinned_empty((batch * per_i,), np.uint8), ctx.pinned_empty((batch * per_t,), np.uint8))
    initial = np.empty((n, m.n_initial), dtype=np.float64) if return_arrays else None
    trace = np.empty((n, T, m.n_dyn), dtype=np.float64) if return_arrays else None
    with open(initial_filename, "wb") as fi, open(transition_filename, "wb") as ft:
        fi.write(header_initial.encode("utf-8"))
        ft.write(header_transition.encode("utf-8"))
        for b0 in range(0, n, batch):
            c = min(batch, n - b0)
            res = native.sample_text_host(ctx, m, c, T, seed, id_first=id_first + b0, want_arrays=return_arrays, buffers=buffers,
                                          first_index=first + b0, max_attempts=1, start=None if grid is None else grid[b0:b0 + c])
            t0 = time.perf_counter()
            fi.write(res["initial"].data)
            ft.write(res["transition"].data)
            st["write_ms"] += (time.perf_counter() - t0) * 1e3
            st["calls"] += 1
            st["library_ms"] += res["host_stats"]["total_ms"]
            for k in ("kernel_ms", "d2h_ms", "scatter_ms"):
                st[k] += res["host_stats"][k]
            st["bytes"] += sum(res["totals"])
            if return_arrays:
                initial[b0:b0 + c] = res["init_val"]
                if m.n_dyn:
                    trace[b0:b0 + c] = res["dyn_val"]
    st["batch"] = batch
    last_text_stats.clear()
    last_text_stats.update(st)
    return initial, trace


def make_valid_name(s):
    """matlab.lang.makeValidName for the label strings of the model files: white space is removed and the
    letter after it capitalised, other invalid characters become '_', a leading non-letter gets an 'x'."""
    s = s.strip()
    s = re.sub(r"\s+([a-z])", lambda mo: mo.group(1).upper(), s)
    s = re.sub(r"\s+", "", s)
    s = re.sub(r"[^A-Za-z0-9_]", "_", s)
    if not s or not s[0].isalpha():
        s = "x" + s
    return s


def _erase(s, chars=('"', "\\")):
    for c in chars:
        s = s.replace(c, "")
    return s


def _read_table(filename, ncol):
    """readtable(..., 'Delimiter', ' ', 'HeaderLines', 1): numeric rows, one header line skipped."""
    with open(filename, "r", encoding="utf-8") as f:
        f.readline()
        data = np.loadtxt(f, dtype=np.float64, ndmin=2)
    if data.size == 0:
        return np.zeros((0, ncol))
    if data.shape[1] != ncol:
        raise ValueError("%s: expected %d columns, found %d" % (filename, ncol, data.shape[1]))
    return data


def _matlab_round(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


UR_SPEED, UR_VERTRATE, UR_HEADING = FT_PER_NM / 3600.0, 1.0 / 60.0, 1.0        # sample2track.m:113-123 (both branches)


def _altitude_grid(min_alt, max_alt):
    """The edges of the altitude directories, step 100 ft (sample2track.m:150-158)."""
    first = np.floor(min_alt - 50.0) if min_alt % 100.0 != 0 else min_alt
    Lgrid = np.arange(first, max_alt + 200.0 + 1e-9, 100.0)
    if Lgrid[0] < 0:
        Lgrid[0] = 0.0
    return Lgrid


def _make_directories(out_dir_parent, Lgrid, geo=None, air=None):
    """Every altitude directory, under every G<g>/A<a> of the initial table for an uncor model that has both (sample2track.m:161-178)."""
    os.makedirs(out_dir_parent, exist_ok=True)
    tops = [()] if geo is None else [("G%i" % g, "A%i" % a) for g in np.unique(geo) for a in np.unique(air)]
    for top in tops:
        for l in Lgrid:
            os.makedirs(os.path.join(out_dir_parent, *top, "%ift" % l), exist_ok=True)


def _track_file_name(rows, track_no, z0, v0):
    """sample2track.m:249 (round: half away from zero)."""
    return "BAYES_t%i_id%i_alt%i_speed%i.csv" % (rows, track_no, _matlab_round(z0), _matlab_round(v0))


def _altitude_directory(Lgrid, z0):
    """The directory of discretize(z0, L) (sample2track.m:263): bin k holds [L(k), L(k + 1)), the last one its top edge as well."""
    k = int(np.searchsorted(Lgrid, z0, side="right")) - 1
    if z0 == Lgrid[-1]:
        k = len(Lgrid) - 2
    if k < 0 or k >= len(Lgrid) - 1:
        raise ValueError("sample2track: initial altitude %g ft is outside the altitude directories" % z0)
    return "%ift" % Lgrid[k]


def _host_csv(xyz):
    """A track's file as the host formats it (sample2track.m:274-279)."""
    return ("time_s,x_ft,y_ft,z_ft\n" + "".join("%i,%0.0f,%0.0f,%0.0f\n" % (t, xyz[t, 0], xyz[t, 1], xyz[t, 2]) for t in range(xyz.shape[0]))).encode("utf-8")


def _t_initial(Ti, names_i, c):
    """T_initial as a dict of columns, speed, acceleration and vertical rate in the tracks' units (sample2track.m:126-128)."""
    T_initial = {name: Ti[:, k].copy() for k, name in enumerate(names_i)}
    for k, ur in ((c.spd, UR_SPEED), (c.acc, UR_SPEED), (c.vr, UR_VERTRATE)):
        if k is not None:
            T_initial[names_i[k]] *= ur
    return T_initial


def sample2track(parameters_filename, initial_filename, transition_filename, num_max_tracks=10000, out_dir_parent=None,
                 label_initial_geographic="G", label_initial_airspace="A", label_initial_altitude="L", label_initial_speed="v",
                 label_initial_acceleration="dotV", label_initial_vertrate="dotH", label_initial_turnrate="dotPsi",
                 label_transition_speed="dotV_t_1_", label_transition_altitude="dotH_t_1_", label_transition_heading="dotPsi_t_1_",
                 isOverwriteZeroBoundaries=False, idxZeroBoundaries=(1, 2, 3), min_altitude_ft=0, rng_seed=42, isPlot=False,
                 write_files=True, verbose=True, ctx=None, text="host"):
    """[is_good, T_initial] = sample2track(parameters_filename, initial_filename, transition_filename, ...)
    (sample2track.m:1-287): 1 Hz dead reckoning of every sampled trajectory (on the GPU), CFIT and speed
    rejection, one `BAYES_t<T>_id<i>_alt<z0>_speed<v0>.csv` per accepted track under
    out_dir_parent/[G<g>/A<a>/]<alt>ft/.  T_initial is returned as a dict of columns (units converted like
    sample2track.m:126-128).  When the initial file holds more than num_max_tracks rows the reference keeps
    randperm(rows, num_max_tracks) of MATLAB's stream; here numpy's RandomState(rng_seed) chooses them.

    text: "host" reads both files with numpy.loadtxt, groups the transition rows on the host and formats every CSV row in Python;
    "device" parses both files on the GPU (native.parse_table, native.tracks_text_host), integrates the tracks from the parsed table where
    it lies and formats the CSV rows there: the same return values, directories, file names and file bytes.  The device reader's grammar is
    narrower than loadtxt's: plain decimal numbers, nan and inf, separated by spaces or tabs; no '#' comments.  Host memory is about the
    transition file plus the CSV text; files larger than memory are out of scope.  last_track_stats says where the time went."""
    if text not in ("host", "device"):
        raise ValueError("sample2track: text must be 'host' or 'device', not %r" % (text,))
    out_dir_parent = out_dir_parent or os.path.join(os.environ.get("AEM_DIR_BAYES", "."), "output", "tracks")
    parameters = em_read(parameters_filename, isOverwriteZeroBoundaries=isOverwriteZeroBoundaries, idxZeroBoundaries=list(idxZeroBoundaries))
    tm = np.asarray(parameters["temporal_map"]).reshape(-1, 2)
    labels_init = [make_valid_name(_erase(s)) for s in parameters["labels_initial"]]                      # :63
    labels_trans = [make_valid_name(_erase(parameters["labels_transition"][int(r[1]) - 1])) for r in tm]  # :64
    names_i = ["id"] + labels_init
    names_t = ["id", "t"] + labels_trans

    def prepare(Ti):
        """What either reader does with the initial table once both files are read: the selection, the columns, the limits."""
        c = types.SimpleNamespace(rows_read=Ti.shape[0])
        if Ti.shape[0] > num_max_tracks:                                                                   # :75-77
            Ti = Ti[np.random.RandomState(int(rng_seed)).permutation(Ti.shape[0])[: int(num_max_tracks)]]
        c.Ti = Ti
        col = lambda names, label: names.index(label) if label in names else None
        c.geo, c.air, c.alt, c.spd, c.acc, c.vr = (col(names_i, l) for l in (
            label_initial_geographic, label_initial_airspace, label_initial_altitude, label_initial_speed, label_initial_acceleration, label_initial_vertrate))
        c.u_acc, c.u_vr, c.u_tr = (col(names_t, l) for l in (label_transition_speed, label_transition_altitude, label_transition_heading))
        for what, k in (("altitude", c.alt), ("speed", c.spd), ("transition speed", c.u_acc), ("transition altitude", c.u_vr),
                        ("transition heading", c.u_tr)):
            if k is None:
                raise ValueError("sample2track: no %s column with the given label" % what)
        b_alt = np.asarray(parameters["boundaries"][labels_init.index(label_initial_altitude)], dtype=np.float64)
        b_spd = np.asarray(parameters["boundaries"][labels_init.index(label_initial_speed)], dtype=np.float64)
        c.min_alt, c.max_alt = float(b_alt[0]), float(b_alt[-1])                                           # :100-101
        c.min_speed, c.max_speed = float(b_spd[0]), float(b_spd[-1])                                       # :104-105
        return c

    reader = _sample2track_device_text if text == "device" else _sample2track_host_text
    c, flags, vmm, lengths, file_bytes, st = reader(ctx, initial_filename, transition_filename, len(names_i), len(names_t), prepare, write_files)
    Ti, num_tracks = c.Ti, c.Ti.shape[0]
    is_good = flags == 0                                                                                   # :243
    Lgrid = _altitude_grid(c.min_alt, c.max_alt)
    is_geo, is_air = c.geo is not None, c.air is not None
    t0 = time.perf_counter()
    if write_files:
        both = "uncor_" in os.path.basename(parameters_filename) and is_geo and is_air
        _make_directories(out_dir_parent, Lgrid, Ti[:, c.geo] if both else None, Ti[:, c.air] if both else None)
    made = set()
    for i in range(num_tracks):
        if not is_good[i]:
            if verbose:
                print("Reject i=%i, CFIT = %i, v = [%0.3f, %0.3f]" % (i + 1, int(flags[i] & 1), vmm[i, 0], vmm[i, 1]))   # :284
            continue
        if not write_files:
            continue
        z0, v0 = Ti[i, c.alt], Ti[i, c.spd] * UR_SPEED
        parts = (["G%i" % Ti[i, c.geo]] if is_geo else []) + (["A%i" % Ti[i, c.air]] if is_air else [])   # :253-260
        out_dir = os.path.join(out_dir_parent, *parts, _altitude_directory(Lgrid, z0))
        if out_dir not in made:
            os.makedirs(out_dir, exist_ok=True)
            made.add(out_dir)
        with open(os.path.join(out_dir, _track_file_name(lengths[i], i + 1, z0, v0)), "wb") as f:          # :274-279
            f.write(file_bytes(i))
    if st is not None:                                      # the device reader's account of the call
        st = dict(st[0], write_ms=(time.perf_counter() - t0) * 1e3, **st[1])
        st.update(tracks=int(num_tracks), accepted=int(is_good.sum()))
        last_track_stats.clear()
        last_track_stats.update(st)
    return is_good, _t_initial(Ti, names_i, c)


def _sample2track_host_text(ctx, initial_filename, transition_filename, ncol_i, ncol_t, prepare, write_files):
    """sample2track(text="host"): both files through numpy.loadtxt, the transition rows grouped on the host, one launch per distinct track
    length (native.sample2track_host); a track's file is formatted in Python from its positions."""
    Ti = _read_table(initial_filename, ncol_i)
    Tt = _read_table(transition_filename, ncol_t)
    c = prepare(Ti)
    Ti, num_tracks = c.Ti, c.Ti.shape[0]
    # group the transition rows by id, in file order (:192-193)
    T_of = {}
    order = np.argsort(Tt[:, 0], kind="stable") if Tt.shape[0] else np.zeros(0, dtype=np.int64)
    ids_sorted = Tt[order, 0] if Tt.shape[0] else np.zeros(0)
    starts = np.flatnonzero(np.r_[True, ids_sorted[1:] != ids_sorted[:-1]]) if ids_sorted.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], ids_sorted.size] if ids_sorted.size else np.zeros(0, dtype=np.int64)
    for s, e in zip(starts, ends):
        T_of[ids_sorted[s]] = order[s:e]
    lens = np.array([len(T_of.get(Ti[i, 0], ())) for i in range(num_tracks)], dtype=np.int64)

    xyz_all = [None] * num_tracks
    flags = np.zeros(num_tracks, dtype=np.uint8)
    vmm = np.zeros((num_tracks, 2))
    context = ctx or native.default_context()
    for T in np.unique(lens):                       # one launch per distinct track length
        sel = np.flatnonzero(lens == T)
        if T == 0:
            for i in sel:                           # no transition rows: the track is its initial point (:196 never runs)
                z0, v0 = Ti[i, c.alt], Ti[i, c.spd] * UR_SPEED
                xyz_all[i] = np.array([[0.0, 0.0, z0]])
                flags[i] = (1 if z0 < 0 else 0) | (2 if (v0 <= c.min_speed * UR_SPEED or v0 >= c.max_speed * UR_SPEED) else 0)
                vmm[i] = (v0, v0)
            continue
        upd = np.stack([Tt[T_of[Ti[i, 0]]][:, [c.u_vr, c.u_acc, c.u_tr]] for i in sel])
        x, f, v = native.sample2track_host(context, Ti[sel, c.alt], Ti[sel, c.spd], upd, UR_SPEED, UR_VERTRATE, UR_HEADING,
                                           c.min_speed, c.max_speed)
        for q, i in enumerate(sel):
            xyz_all[i] = x[q]
        flags[sel], vmm[sel] = f, v
    return c, flags, vmm, lens, lambda i: _host_csv(xyz_all[i]), None


def _read_rows(filename, ctx=None):
    """The bytes of a table file behind its header line: (uint8 array, bytes of the header line).  ctx: into pinned memory of its pool."""
    size = os.path.getsize(filename)
    buf = ctx.pinned_empty((max(size, 1),), np.uint8) if ctx is not None else np.empty(max(size, 1), dtype=np.uint8)
    with open(filename, "rb") as f:
        got = f.readinto(memoryview(buf)[:size]) if size else 0
    data = buf[:got]
    nl = np.flatnonzero(data[: 1 << 16] == 10)
    if nl.size == 0:
        nl = np.flatnonzero(data == 10)
    head = int(nl[0]) + 1 if nl.size else got
    return data[head:], head


def _sample2track_device_text(ctx, initial_filename, transition_filename, ncol_i, ncol_t, prepare, write_files):
    """sample2track(text="device"): both tables parsed, the tracks integrated and the CSV rows formatted on the device (native.parse_table,
    native.tracks_text_host); a track's file is its slice of the device's CSV text, or the host's formatting of its positions where the
    device does not format a coordinate.  Also returns the call's account for last_track_stats, the parts before and after write_ms."""
    ctx = ctx or native.default_context()
    st = {}
    t0 = time.perf_counter()
    rows_i, _ = _read_rows(initial_filename)
    Ti = native.parse_table(ctx, rows_i, ncol_i, header_lines=1)
    rows_t, _ = _read_rows(transition_filename, ctx)
    st["read_ms"] = (time.perf_counter() - t0) * 1e3
    c = prepare(Ti)
    Ti, num_tracks = c.Ti, c.Ti.shape[0]
    # the CSV buffer: sized from the look of the file's first rows, and from the library's exact total when that was too little
    csv_cap = None
    if write_files:
        head = rows_t[: 1 << 20]
        per_line = head.size / max(int(np.count_nonzero(head == 10)), 1)
        share = num_tracks / max(c.rows_read, 1)
        csv_cap = int(num_tracks * 64 + rows_t.size / max(per_line, 1.0) * share * 30) + (1 << 16)
    args = (ctx, rows_t, ncol_t, (c.u_vr, c.u_acc, c.u_tr), Ti[:, 0], Ti[:, c.alt], Ti[:, c.spd], UR_SPEED, UR_VERTRATE, UR_HEADING,
            c.min_speed, c.max_speed)
    t0 = time.perf_counter()
    try:
        res = native.tracks_text_host(*args, want_csv=write_files, csv_cap=csv_cap)
    except native.L.EmgpuError as e:
        if e.code != native.L.ERR_EVENT_CAP:
            raise
        res = native.tracks_text_host(*args, want_csv=write_files, csv_cap=int(e.totals[0]))
    host_xyz = None
    if write_files and res["totals"]["host_formatted"]:     # coordinates the device does not format: those files are written as the host path writes them
        host_xyz = native.tracks_text_host(*args, want_csv=False, want_xyz=True)["xyz"]
    st["library_ms"] = (time.perf_counter() - t0) * 1e3
    after = {"library_call_ms": res["host_stats"]["total_ms"], "bytes_transition": int(rows_t.size)}
    after.update({k + "_ms": v for k, v in res["phase_ms"].items()})
    after.update(res["totals"])
    csv = res["csv"]
    offs = res["offsets"].astype(np.int64).tolist() if write_files else None

    def file_bytes(i):
        return csv[offs[i]:offs[i + 1]].data if offs[i + 1] > offs[i] else _host_csv(host_xyz[i])
    return c, res["flags"], res["speed_minmax"], res["lengths"], file_bytes, (st, after)
