"""ctypes binding of the MI355X back end (liblmc_hip.so, C ABI in include/lmc_abi.h).

The package is plumbing around the C ABI: it loads the HIP library (and fails loudly if it is missing or if no GPU is
usable); it never computes anything on the CPU.  Import with importlib.import_module("langevin-mcmc_amd")."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("LMC_LIB") or os.path.join(_HERE, "liblmc_hip.so")  # LMC_LIB: A/B builds of the same library (scripts/)
vp = ctypes.c_void_p
c_ll = ctypes.c_longlong


class SceneDesc(ctypes.Structure):
    _fields_ = [
        ("scene_xml", ctypes.c_char_p),
        ("force_diffuse", ctypes.c_int),
        ("max_depth", ctypes.c_int),
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("seed_offset", ctypes.c_int),
        ("device", ctypes.c_int),
        ("use_gradient", ctypes.c_int),
    ]


def P(a):
    return a.ctypes.data_as(vp)


_lib = None


def lib():
    """The loaded HIP library; raises if it has not been built (run `python __graft_entry__.py`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP extension missing: %s (build with `python __graft_entry__.py`); there is no CPU fallback" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.lmc_last_error.restype = ctypes.c_char_p
        L.lmc_create.restype = vp
        L.lmc_create.argtypes = [ctypes.POINTER(SceneDesc)]
        L.lmc_destroy.argtypes = [vp]
        L.lmc_info.argtypes = [vp, vp]
        L.lmc_scene_params.argtypes = [vp, vp]
        L.lmc_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_double]
        L.lmc_chains_init.argtypes = [vp, c_ll, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_ll, c_ll]
        L.lmc_init_result.argtypes = [vp, vp, vp]
        L.lmc_chains_step.argtypes = [vp, ctypes.c_int]
        L.lmc_sync.argtypes = [vp]
        L.lmc_film_read.argtypes = [vp, vp]
        L.lmc_film_clear.argtypes = [vp]
        L.lmc_stats.argtypes = [vp, vp, vp]
        L.lmc_chain_summary.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int]
        L.lmc_step_timing.argtypes = [vp, vp, vp]
        L.lmc_relocation_stats.argtypes = [vp, vp]
        if hasattr(L, "lmc_resident_stats"):  # (an A/B library built from an older tree, LMC_LIB, has no resident schedule)
            L.lmc_resident_stats.argtypes = [vp, vp, vp]
        if hasattr(L, "lmc_relocation_skipped"):  # (an older A/B build selected with LMC_LIB lacks it)
            L.lmc_relocation_skipped.argtypes = [vp]
            L.lmc_relocation_skipped.restype = c_ll
        L.lmc_kernel_timing.argtypes = [vp, vp]
        L.lmc_kernel_timing_split.argtypes = [vp, vp]
        L.lmc_get_option.argtypes = [vp, ctypes.c_char_p, vp]
        L.lmc_output_name.argtypes = [vp]
        L.lmc_output_name.restype = ctypes.c_char_p
        L.lmc_image_read.argtypes = [ctypes.c_char_p, vp, vp, vp]
        L.lmc_image_write_exr.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int]
        L.lmc_direct_lighting.argtypes = [vp, ctypes.c_int]
        L.lmc_direct_read.argtypes = [vp, vp]
        L.lmc_path_trace.argtypes = [vp, ctypes.c_int]
        L.lmc_bidir_mc.argtypes = [vp, ctypes.c_int]
        if hasattr(L, "lmc_mc_render"):  # (an A/B library built from an older tree, LMC_LIB, has no mc integrator)
            L.lmc_mc_render.argtypes = [vp, ctypes.c_int, c_ll, c_ll]
            L.lmc_mc_read.argtypes = [vp, vp]
            L.lmc_mc_stats.argtypes = [vp, vp]
        if hasattr(L, "lmc_mc_accumulate"):  # (an A/B library built from an older tree, LMC_LIB, has no exact mc film)
            L.lmc_mc_accumulate.argtypes = [vp, ctypes.c_int, c_ll, c_ll]
            L.lmc_mc_coverage.argtypes = [vp, vp, ctypes.c_int]
            L.lmc_mc_read_fixed.argtypes = [vp, vp]
            L.lmc_mc_overflow.argtypes = [vp, vp]
            L.lmc_group_mc_render.argtypes = [vp, ctypes.c_int, ctypes.c_int, c_ll, c_ll]
            L.lmc_group_mc_accumulate.argtypes = [vp, ctypes.c_int, ctypes.c_int, c_ll, c_ll]
            L.lmc_mc_save.argtypes = [vp, ctypes.c_char_p]
            L.lmc_mc_load.argtypes = [vp, ctypes.c_char_p]
            L.lmc_mc_file_info.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_ll]
            L.lmc_mc_file_info.restype = c_ll
            L.lmc_mc_coverage_probe.argtypes = [vp, ctypes.c_int, c_ll, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp]
            L.lmc_mc_chunks_probe.argtypes = [c_ll, c_ll, c_ll, c_ll, vp, ctypes.c_int]
        if hasattr(L, "lmc_mc_layer_info"):  # (an A/B library built from an older tree, LMC_LIB, has no layered mc film)
            L.lmc_mc_layer_info.argtypes = [vp, vp, vp, vp, ctypes.c_int]
            L.lmc_mc_read_layer.argtypes = [vp, ctypes.c_int, vp]
            L.lmc_mc_read_layer_fixed.argtypes = [vp, ctypes.c_int, vp]
        L.lmc_stream_probe.argtypes = [c_ll, ctypes.c_int]
        L.lmc_grad_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp]
        L.lmc_trace.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        L.lmc_occluded.argtypes = [vp, ctypes.c_int, vp, vp]
        L.lmc_rng_probe.argtypes = [ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp]
        L.lmc_kd_probe.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_float, ctypes.c_int, vp, vp, vp]
        L.lmc_lean_query_probe.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [vp] * 11
        L.lmc_gauss_probe.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_float, ctypes.c_float, vp, vp, vp]
        L.lmc_comm_unique_id.argtypes = [vp]
        L.lmc_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.lmc_film_allreduce.argtypes = [vp]
        L.lmc_film_device_ptr.argtypes = [vp, vp]
        L.lmc_film_device_ptr.restype = vp
        L.lmc_comm_allreduce_f64.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int]
        L.lmc_comm_barrier.argtypes = [vp]
        L.lmc_host_issue_timing.argtypes = [vp, vp, vp]
        L.lmc_group_info.argtypes = [vp, ctypes.c_int, vp]
        if hasattr(L, "lmc_checkpoint_save"):  # (an A/B library built from an older tree, LMC_LIB, has no checkpoints)
            L.lmc_checkpoint_save.argtypes = [vp, ctypes.c_char_p]
            L.lmc_checkpoint_load.argtypes = [vp, ctypes.c_char_p]
            L.lmc_group_checkpoint_save.argtypes = [vp, ctypes.c_int, ctypes.c_char_p]
            L.lmc_group_checkpoint_load.argtypes = [vp, ctypes.c_int, ctypes.c_char_p]
            L.lmc_checkpoint_info.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_ll]
            L.lmc_checkpoint_info.restype = c_ll
        if hasattr(L, "lmc_film_read_fixed"):  # (an A/B library built from an older tree, LMC_LIB, has no exact film)
            L.lmc_film_read_fixed.argtypes = [vp, vp]
            L.lmc_film_overflow.argtypes = [vp, vp]
            L.lmc_film_splat_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp]
        if hasattr(L, "lmc_scan_probe"):  # (an A/B library built from an older tree, LMC_LIB, has no list probes)
            ci, cu = ctypes.c_int, ctypes.c_uint
            L.lmc_scan_probe.argtypes = [ci, vp, vp]
            L.lmc_radix_sort_probe.argtypes = [ci, ci, vp, vp, vp]
            L.lmc_sort_by_technique_probe.argtypes = [ci, vp, ci, vp, ci, vp]
            L.lmc_build_lists_probe.argtypes = [ci, vp, ci, cu, ci, vp, vp, vp, vp, vp]
            L.lmc_bins_compact_probe.argtypes = [ci, vp, vp, ci, vp, ci, vp, vp]
            L.lmc_split_list_probe.argtypes = [ci, vp, ci, ci, ci, vp, vp]
            L.lmc_cache_push_probe.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp]
            L.lmc_reloc_plan_probe.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp]
            L.lmc_chain_slots.argtypes = [vp, vp, vp]
        if hasattr(L, "lmc_coop_plan_probe"):  # (an A/B library built from an older tree, LMC_LIB, has no work-list probes of the cooperative launches)
            ci = ctypes.c_int
            L.lmc_mala_grad_list_probe.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp]
            L.lmc_h2_hess_list_probe.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp]
            L.lmc_h2_gauss_list_probe.argtypes = [ci, vp, vp, vp, vp, vp, ci, ctypes.c_float, ci, vp, vp, vp, ci, vp, vp]
            L.lmc_coop_plan_probe.argtypes = [ci, ci, vp, vp]
        if hasattr(L, "lmc_shade_probe"):  # (an A/B library built from an older tree, LMC_LIB, has no shading probe)
            ci = ctypes.c_int
            L.lmc_shade_probe.argtypes = [ci, ci, ci, vp, ci, vp, vp, vp, c_ll, ci, ci, vp, vp, vp, vp]
        if hasattr(L, "lmc_chain_rows"):  # (an A/B library built from an older tree, LMC_LIB, has no chain diagnostics)
            L.lmc_chain_rows.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, vp]
            L.lmc_chain_trace_begin.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int]
            L.lmc_chain_trace_read.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
            L.lmc_chain_trace_end.argtypes = [vp]
            L.lmc_step_table.argtypes = [vp, vp, ctypes.c_int]
        if hasattr(L, "lmc_film_layer_info"):  # (an A/B library built from an older tree, LMC_LIB, has no layered MLT film)
            ci = ctypes.c_int
            L.lmc_film_layer_info.argtypes = [vp, vp, vp, vp, ci]
            L.lmc_film_read_layer.argtypes = [vp, ci, vp]
            L.lmc_film_read_layer_fixed.argtypes = [vp, ci, vp]
            L.lmc_chain_splats.argtypes = [vp, vp, ci, ci, vp, vp]
            L.lmc_film_layer_splat_probe.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _err():
    return lib().lmc_last_error().decode()


SPLAT_WORDS, SPLAT_MAX_ENTRIES = 6, 85  # include/lmc_abi.h LMC_SPLAT_WORDS, LMC_SPLAT_MAX_ENTRIES


def film_layer_of(mode, c, l):
    """The layer of technique (c, l) = (camDepth, lightDepth) in a layered film ("mc_layers" and "film_layers" share the numbering): mode 1 (by
    path length L = c + l - 1) L - 1, mode 2 (by technique) (L - 1)(L + 2) / 2 + l; -1: no such technique.  A film of maxdepth D holds the layers below
    film_layer_count(mode, D)."""
    L = c + l - 1
    if mode not in (1, 2):
        raise ValueError("film_layer_of: mode is 1 (by path length) or 2 (by technique)")
    if c < 1 or l < 0 or L < 1:
        return -1
    return L - 1 if mode == 1 else (L - 1) * (L + 2) // 2 + l


def film_layer_count(mode, max_depth):
    if mode not in (0, 1, 2):
        raise ValueError("film_layer_count: mode is 0 (off), 1 (by path length) or 2 (by technique)")
    return 0 if mode == 0 else max_depth if mode == 1 else max_depth * (max_depth + 3) // 2


class Renderer:
    """One scene resident on one GPU; mirrors MLT() of the reference (mlt.cpp:20-214) step by step."""

    def __init__(self, xml, force_diffuse=0, max_depth=0, width=0, height=0, seed_offset=-1, device=0, use_gradient=1):
        L = lib()
        self._xml = os.fsencode(xml)
        d = SceneDesc(self._xml, force_diffuse, max_depth, width, height, seed_offset, device, use_gradient)
        h = L.lmc_create(ctypes.byref(d))
        if not h:
            raise RuntimeError("lmc_create failed: " + _err())
        self.h = vp(h)
        info = (ctypes.c_int * 8)()
        L.lmc_info(self.h, info)
        (self.width, self.height, self.num_tris, self.max_depth, self.num_nodes, self.bvh_depth, self.num_lights, self.mala) = list(info)
        self.num_chains = 0

    def close(self):
        if self.h:
            lib().lmc_destroy(self.h)
            self.h = None

    def set_option(self, name, value):
        if lib().lmc_set_option(self.h, name.encode(), float(value)) != 0:
            raise RuntimeError(_err())

    def get_option(self, name):
        v = ctypes.c_double()
        if lib().lmc_get_option(self.h, name.encode(), ctypes.byref(v)) != 0:
            raise RuntimeError(_err())
        return v.value

    def scene_params(self):
        s = np.zeros(38, np.float32)
        lib().lmc_scene_params(self.h, P(s))
        return s

    def init_chains(self, num_init, n_chains_total, init_threads, per_chain, extra=0, chain_begin=0, chain_end=None):
        if chain_end is None:
            chain_end = n_chains_total
        if lib().lmc_chains_init(self.h, num_init, n_chains_total, init_threads, chain_begin, chain_end, per_chain, extra) != 0:
            raise RuntimeError("lmc_chains_init failed: " + _err())
        self.num_chains = chain_end - chain_begin
        self.num_chains_total = n_chains_total
        n = ctypes.c_float()
        nc = c_ll()
        lib().lmc_init_result(self.h, ctypes.byref(n), ctypes.byref(nc))
        self.normalization = n.value
        return n.value, nc.value

    def step(self, n):
        if lib().lmc_chains_step(self.h, n) != 0:
            raise RuntimeError("lmc_chains_step failed: " + _err())

    def save_checkpoint(self, path):
        """The chains, caches, counters and film as they are between two step() calls, into one file (written as path + ".tmp", then renamed);
        changes nothing in the renderer."""
        if lib().lmc_checkpoint_save(self.h, os.fsencode(path)) != 0:
            raise RuntimeError("lmc_checkpoint_save failed: " + _err())
        return getattr(self, "normalization", None)

    def load_checkpoint(self, path):
        """Takes the place of init_chains on a renderer created from the same scene, overrides and options: the render a save_checkpoint (of a
        Renderer or a Group of any size) wrote goes on exactly where it stopped.  Returns the normalization and sets num_chains."""
        if lib().lmc_checkpoint_load(self.h, os.fsencode(path)) != 0:
            raise RuntimeError("lmc_checkpoint_load failed: " + _err())
        self.num_chains = self.num_chains_total = checkpoint_info(path)["n_chains_total"]
        n = ctypes.c_float()
        lib().lmc_init_result(self.h, ctypes.byref(n), None)
        self.normalization = n.value
        return n.value

    def sync(self):
        if lib().lmc_sync(self.h) != 0:
            raise RuntimeError(_err())

    def film(self):
        f = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_film_read(self.h, P(f)) != 0:
            raise RuntimeError(_err())
        return f

    def film_clear(self):
        """zeroes the film (exact mode: the words and the overflow counter; "film_layers": every layer); the chains go on from where they are"""
        if lib().lmc_film_clear(self.h) != 0:
            raise RuntimeError(_err())

    def film_fixed(self):
        """Exact mode (set_option("film_exact", 1) before init_chains / load_checkpoint): the film's raw words, int64 [H, W, 3], one unit =
        2^-32 of the float film's unit; film() is np.float32(np.float64(words) * 2.0**-32).  Raises in float mode."""
        f = np.zeros((self.height, self.width, 3), np.int64)
        if lib().lmc_film_read_fixed(self.h, P(f)) != 0:
            raise RuntimeError(_err())
        return f

    def film_overflow(self):
        """Exact mode: splats dropped because a component was 2^30 or more since the film was last cleared (0 in float mode)."""
        n = c_ll()
        if lib().lmc_film_overflow(self.h, ctypes.byref(n)) != 0:
            raise RuntimeError(_err())
        return int(n.value)

    # ---- multi-GPU (include/lmc_abi.h): in-library RCCL sum of the device films
    def comm_init(self, n_ranks, rank, id128):
        buf = (ctypes.c_ubyte * 128).from_buffer_copy(bytes(id128))
        if lib().lmc_comm_init(self.h, n_ranks, rank, buf) != 0:
            raise RuntimeError("lmc_comm_init failed: " + _err())

    def film_allreduce(self):
        if lib().lmc_film_allreduce(self.h) != 0:
            raise RuntimeError("lmc_film_allreduce failed: " + _err())

    def comm_allreduce(self, values, op="sum"):
        """host doubles reduced over the ranks of the job's communicator (op: sum / max / min); returns a list"""
        v = (ctypes.c_double * len(values))(*[float(x) for x in values])
        if lib().lmc_comm_allreduce_f64(self.h, v, len(values), {"sum": 0, "max": 1, "min": 2}[op]) != 0:
            raise RuntimeError("lmc_comm_allreduce_f64 failed: " + _err())
        return list(v)

    def comm_gather(self, value, rank, world):
        """every rank's scalar, in rank order, on every rank (a sum of one-hot vectors over the job's communicator)"""
        return self.comm_allreduce([float(value) if k == rank else 0.0 for k in range(world)], "sum")

    def comm_barrier(self):
        if lib().lmc_comm_barrier(self.h) != 0:
            raise RuntimeError("lmc_comm_barrier failed: " + _err())

    def host_issue_timing(self):
        """(ms of host time spent queueing this context's steps since the last call, steps covered)"""
        ms, n = ctypes.c_double(), c_ll()
        if lib().lmc_host_issue_timing(self.h, ctypes.byref(ms), ctypes.byref(n)) != 0:
            raise RuntimeError(_err())
        return ms.value, n.value

    def direct_lighting(self, direct_spp):
        """DirectLighting pre-pass (direct.cpp); returns the un-normalised direct buffer [H, W, 3]."""
        if lib().lmc_direct_lighting(self.h, int(direct_spp)) != 0:
            raise RuntimeError(_err())
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_direct_read(self.h, P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def path_trace(self, spp):
        """Unidirectional path tracing with next-event estimation over the scene's full depth range (cross-check estimator)."""
        if lib().lmc_path_trace(self.h, int(spp)) != 0:
            raise RuntimeError(_err())
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_direct_read(self.h, P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def bidir_mc(self, spp):
        """Plain Monte Carlo over bidirectional samples (path length >= 3): radiance image [H, W, 3]."""
        if lib().lmc_bidir_mc(self.h, int(spp)) != 0:
            raise RuntimeError(_err())
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_direct_read(self.h, P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def mc_render(self, spp, streams=None):
        """The scene's "mc" integrator (PathTrace): spp samples per pixel, bidirectional or not as the scene says (set_option "bidirectional"
        overrides it); radiance image [H, W, 3], already weighted by 1 / spp.  streams=(begin, end): only those stream ids of
        [0, nTiles * spp) (end -1: to the last one); the films of disjoint ranges sum to the film of their union.  After
        set_option("mc_film_exact", 1) the film is the fixed-point sum of the unweighted contributions (mc_film_fixed) and what is returned is
        that sum divided by spp; mc_accumulate then adds further ranges."""
        begin, end = (0, -1) if streams is None else (int(streams[0]), int(streams[1]))
        if lib().lmc_mc_render(self.h, int(spp), begin, end) != 0:
            raise RuntimeError(_err())
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_mc_read(self.h, P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def mc_stats(self):
        """(paths traced, contributions splatted) of the last mc_render; with the exact mc film: since the film was last cleared"""
        o = (c_ll * 2)()
        if lib().lmc_mc_stats(self.h, o) != 0:
            raise RuntimeError(_err())
        return int(o[0]), int(o[1])

    # ---- the exact mc film (set_option("mc_film_exact", 1) before mc_render; include/lmc_abi.h "Exact mc film")
    def mc_film(self):
        """the mc film as mc_render returned it, read again (exact mode: the words divided by the latest call's spp)"""
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_mc_read(self.h, P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def mc_accumulate(self, spp, streams=None):
        """Adds the stream ids streams=(begin, end) of [0, nTiles * spp) to the exact mc film without clearing it; spp becomes the read divisor.
        A range that overlaps what the film holds raises and leaves the film as it was.  Returns the film like mc_render."""
        begin, end = (0, -1) if streams is None else (int(streams[0]), int(streams[1]))
        if lib().lmc_mc_accumulate(self.h, int(spp), begin, end) != 0:
            raise RuntimeError("lmc_mc_accumulate failed: " + _err())
        return self.mc_film()

    def mc_film_fixed(self):
        """the exact mc film's raw words, int64 [H, W, 3] (unit 2^-32, unweighted); raises in float mode"""
        f = np.zeros((self.height, self.width, 3), np.int64)
        if lib().lmc_mc_read_fixed(self.h, P(f)) != 0:
            raise RuntimeError("lmc_mc_read_fixed failed: " + _err())
        return f

    def mc_overflow(self):
        """contributions the exact mc film dropped by its range rule (a component |v| >= 2^30) since it was last cleared; 0 in float mode"""
        n = c_ll()
        if lib().lmc_mc_overflow(self.h, ctypes.byref(n)) != 0:
            raise RuntimeError(_err())
        return int(n.value)

    def mc_coverage(self):
        """the stream ids the exact mc film holds: a list of disjoint, merged, ascending (begin, end) pairs"""
        n = lib().lmc_mc_coverage(self.h, None, 0)
        if n < 0:
            raise RuntimeError(_err())
        o = (c_ll * (2 * max(n, 1)))()
        lib().lmc_mc_coverage(self.h, o, n)
        return [(int(o[2 * k]), int(o[2 * k + 1])) for k in range(n)]

    def mc_save(self, path):
        """the exact mc film with its divisor, counters and coverage as one file (written to path + ".tmp", then renamed)"""
        if lib().lmc_mc_save(self.h, os.fsencode(path)) != 0:
            raise RuntimeError("lmc_mc_save failed: " + _err())

    def mc_load(self, path):
        """Replaces the exact mc film by a file's (set_option("mc_film_exact", 1) first); a file of another scene, film size, depth range, seed offset or
        generator raises naming the field and leaves the context as it was.  mc_accumulate then continues the render."""
        if lib().lmc_mc_load(self.h, os.fsencode(path)) != 0:
            raise RuntimeError("lmc_mc_load failed: " + _err())

    # ---- the layered mc film (set_option("mc_layers", 1 | 2) before mc_render; include/lmc_abi.h "Layered mc film")
    def mc_layer_info(self):
        """(mode, layers) of the mc film the renderer holds: mode 0 / 1 (by path length) / 2 (by technique), layers a list of (L, -1) in length
        mode and of (camDepth, lightDepth) in technique mode, [] for an unlayered film"""
        mode, n = ctypes.c_int(), ctypes.c_int()
        if lib().lmc_mc_layer_info(self.h, ctypes.byref(mode), ctypes.byref(n), None, 0) != 0:
            raise RuntimeError(_err())
        cl = (ctypes.c_int * (2 * max(n.value, 1)))()
        if lib().lmc_mc_layer_info(self.h, ctypes.byref(mode), ctypes.byref(n), cl, n.value) != 0:
            raise RuntimeError(_err())
        return mode.value, [(int(cl[2 * k]), int(cl[2 * k + 1])) for k in range(n.value)]

    def mc_layer(self, k):
        """layer k of the layered mc film as mc_film() returns the whole, float32 [H, W, 3]"""
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_mc_read_layer(self.h, int(k), P(out)) != 0:
            raise RuntimeError("lmc_mc_read_layer failed: " + _err())
        return out

    def mc_layer_fixed(self, k):
        """layer k's raw words, int64 [H, W, 3]; raises in float mode"""
        f = np.zeros((self.height, self.width, 3), np.int64)
        if lib().lmc_mc_read_layer_fixed(self.h, int(k), P(f)) != 0:
            raise RuntimeError("lmc_mc_read_layer_fixed failed: " + _err())
        return f

    def mc_layers(self):
        """every layer, float32 [n, H, W, 3]; in float mode mc_film() is their float sum in layer order"""
        n = len(self.mc_layer_info()[1])
        if n == 0:
            raise RuntimeError("mc_layers: the renderer holds no layered mc film (set_option(\"mc_layers\", 1 or 2) before mc_render)")
        return np.stack([self.mc_layer(k) for k in range(n)])

    def mc_layers_fixed(self):
        """every layer's raw words, int64 [n, H, W, 3]; their sum over the first axis is mc_film_fixed()"""
        n = len(self.mc_layer_info()[1])
        if n == 0:
            raise RuntimeError("mc_layers_fixed: the renderer holds no layered mc film (set_option(\"mc_layers\", 1 or 2) before mc_render)")
        return np.stack([self.mc_layer_fixed(k) for k in range(n)])

    def stats(self):
        s = (c_ll * 8)()
        w = ctypes.c_double()
        if lib().lmc_stats(self.h, s, ctypes.byref(w)) != 0:
            raise RuntimeError(_err())
        keys = ["steps", "largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets", "cacheReadyMask"]
        d = dict(zip(keys, list(s)))
        d["weightSum"] = w.value
        return d

    def relocation_stats(self):
        """None when chain relocation is off; else relocations run, chains moved by the last one, technique breaks between adjacent slots, slots"""
        o = (c_ll * 4)()
        r = lib().lmc_relocation_stats(self.h, o)
        if r == -1:
            return None
        if r != 0:
            raise RuntimeError(_err())
        return dict(relocations=o[0], moved=o[1], breaks=o[2], slots=o[3], skipped=int(lib().lmc_relocation_skipped(self.h)) if hasattr(lib(), "lmc_relocation_skipped") else 0)

    def resident_stats(self):
        """The resident schedule (set_option("resident_steps", K)) since init_chains: resident launches, chain-steps they advanced, lock steps run,
        K in force (after the cap), HIP-event ms of the resident launches, and the guard: steps that would have needed a gradient / cache push (0)"""
        o = (c_ll * 4)()
        ms = ctypes.c_double()
        if lib().lmc_resident_stats(self.h, o, ctypes.byref(ms)) != 0:
            raise RuntimeError(_err())
        return dict(launches=o[0], chain_steps=o[1], lock_steps=o[2], k=o[3], kernel_ms=ms.value, guard=int(self.get_option("resident_guard")))

    def chain_slots(self):
        """Test probe: (slot_of[chain], chain_id[slot]) of the resident chains, or None when chain relocation is off"""
        so, ci = np.full(self.num_chains, -1, np.int32), np.full(self.num_chains, -1, np.int32)
        r = lib().lmc_chain_slots(self.h, P(so), P(ci))
        if r == -1:
            return None
        if r != 0:
            raise RuntimeError(_err())
        return so, ci

    def summary(self, which=0):
        n = self.num_chains  # which = 0: current states, 1: init states -- of this rank's chains
        out = np.zeros((n, 32), np.float32)
        if lib().lmc_chain_summary(self.h, which, P(out), 32) < 0:
            raise RuntimeError(_err())
        return out

    # ---- chain diagnostics (include/lmc_abi.h "Chain diagnostics")
    def chain_rows(self, ids, which=0):
        """[n, 48] float32: the rows of the chains `ids` (GLOBAL chain ids of this renderer's range), gathered on the device; which = 0 current
        states, 1 init states.  Words 0..15 as summary(), 16..39 pss[0..23], 40 step kind (-1 outside a trace), 41 adjacentReject, 42 flags."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros((len(ids), ROW_WORDS), np.float32)
        if lib().lmc_chain_rows(self.h, which, P(ids), len(ids), P(out)) != 0:
            raise RuntimeError(_err())
        return out

    def trace_chains(self, ids, capacity):
        """Open a trace of the chains `ids`: every lock step from now on records their rows on the device, up to `capacity` steps between reads."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if lib().lmc_chain_trace_begin(self.h, P(ids), len(ids), int(capacity)) != 0:
            raise RuntimeError(_err())
        self._trace_n = len(ids)

    def trace_read(self):
        """(first_step, dropped, rows[steps, n, 48]) of the open trace; empties the buffer, recording goes on"""
        first, dropped, n_steps = c_ll(), c_ll(), ctypes.c_int()
        if lib().lmc_chain_trace_read(self.h, None, 0, ctypes.byref(first), ctypes.byref(n_steps), ctypes.byref(dropped)) != 0:
            raise RuntimeError(_err())
        rows = np.zeros((n_steps.value, self._trace_n, ROW_WORDS), np.float32)
        if lib().lmc_chain_trace_read(self.h, P(rows), n_steps.value, ctypes.byref(first), ctypes.byref(n_steps), ctypes.byref(dropped)) != 0:
            raise RuntimeError(_err())
        return first.value, dropped.value, rows

    def trace_end(self):
        if lib().lmc_chain_trace_end(self.h) != 0:
            raise RuntimeError(_err())

    def chain_splats(self, ids, cap=SPLAT_MAX_ENTRIES):
        """(counts[n] int32, entries[n, cap, 6] float32): the pending splat lists of the chains `ids` (GLOBAL chain ids of this renderer's range),
        gathered on the device.  An entry: x, y, r, g, b as stored and its label camDepth * 16 + lightDepth (-1 unless "film_layers" is set);
        entries from min(counts[k], cap) on are zero."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        cap = int(cap)
        if len(ids) == 0:
            raise ValueError("chain_splats: at least one chain id expected")
        if not 1 <= cap <= SPLAT_MAX_ENTRIES:
            raise ValueError("chain_splats: cap is 1 .. %d entries per chain" % SPLAT_MAX_ENTRIES)
        out = np.zeros((len(ids), cap, SPLAT_WORDS), np.float32)
        counts = np.zeros(len(ids), np.int32)
        if lib().lmc_chain_splats(self.h, P(ids), len(ids), cap, P(out), P(counts)) != 0:
            raise RuntimeError(_err())
        return counts, out

    # ---- the layered MLT film (set_option("film_layers", 1 | 2) and ("film_exact", 1) before init_chains; include/lmc_abi.h "Layered MLT film")
    def film_layer_info(self):
        """(mode, layers) of the MLT film the renderer holds: mode 0 / 1 (by path length) / 2 (by technique), layers a list of (L, -1) in length
        mode and of (camDepth, lightDepth) in technique mode, [] for an unlayered film"""
        mode, n = ctypes.c_int(), ctypes.c_int()
        if lib().lmc_film_layer_info(self.h, ctypes.byref(mode), ctypes.byref(n), None, 0) != 0:
            raise RuntimeError(_err())
        cl = (ctypes.c_int * (2 * max(n.value, 1)))()
        if lib().lmc_film_layer_info(self.h, ctypes.byref(mode), ctypes.byref(n), cl, n.value) != 0:
            raise RuntimeError(_err())
        return mode.value, [(int(cl[2 * k]), int(cl[2 * k + 1])) for k in range(n.value)]

    def film_layer(self, k):
        """layer k of the layered MLT film as film() returns the whole, float32 [H, W, 3], un-normalised"""
        if int(k) != k:
            raise TypeError("film_layer: an integer layer index expected")
        out = np.zeros((self.height, self.width, 3), np.float32)
        if lib().lmc_film_read_layer(self.h, int(k), P(out)) != 0:
            raise RuntimeError("lmc_film_read_layer failed: " + _err())
        return out

    def film_layer_fixed(self, k):
        """layer k's raw words, int64 [H, W, 3]"""
        if int(k) != k:
            raise TypeError("film_layer_fixed: an integer layer index expected")
        f = np.zeros((self.height, self.width, 3), np.int64)
        if lib().lmc_film_read_layer_fixed(self.h, int(k), P(f)) != 0:
            raise RuntimeError("lmc_film_read_layer_fixed failed: " + _err())
        return f

    def film_layers_fixed(self):
        """every layer's raw words, int64 [n, H, W, 3]; their sum over the first axis is film_fixed()"""
        n = len(self.film_layer_info()[1])
        if n == 0:
            raise RuntimeError("film_layers_fixed: the renderer holds no layered film (set_option(\"film_layers\", 1 or 2) and (\"film_exact\", 1) before init_chains)")
        return np.stack([self.film_layer_fixed(k) for k in range(n)])

    def step_table(self, clear=False):
        """int64 [3, 13, 13, 2]: [kind - 1 (large, generic small, lean small)][c][l][chain-steps | accepted], counted while
        set_option("step_table", 1) is in force"""
        out = np.zeros((3, 13, 13, 2), np.int64)
        if lib().lmc_step_table(self.h, P(out), 1 if clear else 0) != 0:
            raise RuntimeError(_err())
        return out

    def step_timing(self):
        ms = ctypes.c_double()
        n = c_ll()
        if lib().lmc_step_timing(self.h, ctypes.byref(ms), ctypes.byref(n)) != 0:
            raise RuntimeError(_err())
        return ms.value, n.value

    def kernel_timing(self):
        """(ms in the lean small-step kernel, ms in the large/generic launches) over the interval of the last
        step_timing() call, and the cumulative number of chain-steps the lean kernel has run."""
        out = (ctypes.c_double * 3)()
        if lib().lmc_kernel_timing(self.h, out) != 0:
            raise RuntimeError(_err())
        return out[0], out[1], int(out[2])

    def kernel_timing_split(self):
        """the three step launches separately over the interval of the last step_timing() call: ms in the lean small-step kernel,
        in the large-step launch and in the generic small-step launch (cache-filling gradient steps / every H2MC small step), plus
        the cumulative number of chain-steps the lean kernel has run"""
        out = (ctypes.c_double * 4)()
        if lib().lmc_kernel_timing_split(self.h, out) != 0:
            raise RuntimeError(_err())
        return {"lean_ms": out[0], "large_ms": out[1], "generic_ms": out[2], "lean_steps": int(out[3])}

    def lean_info(self):
        """The lean small-step launch of this context (lmc_lean_info): leaves of the tree by triangle count, stack need, LDS stack words and
        which instantiation of the kernel it takes"""
        out = (ctypes.c_int * 16)()
        L = lib()
        L.lmc_lean_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        if L.lmc_lean_info(self.h, out) != 0:
            raise RuntimeError(_err())
        v = list(out)
        return dict(leaf_hist=v[:8], stack_need=v[8], stack_words=v[9], lds=v[10], glossy=v[11], lightless=v[12], quant=v[13], tight=v[14], block=v[15])

    def trace(self, rays):
        rays = np.ascontiguousarray(rays, np.float32)
        n = len(rays)
        prim = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        if lib().lmc_trace(self.h, n, P(rays), P(prim), P(t)) != 0:
            raise RuntimeError(_err())
        return prim, t

    def occluded(self, rays):
        rays = np.ascontiguousarray(rays, np.float32)
        occ = np.zeros(len(rays), np.int32)
        if lib().lmc_occluded(self.h, len(rays), P(rays), P(occ)) != 0:
            raise RuntimeError(_err())
        return occ


class Group:
    """In-process ranks: the given Renderers (one per GPU, or several on one GPU for bring-up / tests) become ranks 0 .. n-1 of ONE job
    (lmc_group_chains_init / lmc_group_chains_step): MLTInit sharded by init stream, chains split into contiguous equal ranges, the
    global cache's pushes exchanged every step -- the same trajectories as a single rank holding all the chains."""

    def __init__(self, renderers):
        self.rens = list(renderers)
        self._arr = (vp * len(self.rens))(*[r.h for r in self.rens])

    def _check_film_modes(self):
        modes = [int(r.get_option("film_exact")) for r in self.rens]
        if len(set(modes)) > 1:
            raise RuntimeError("Group: the members differ in film_exact (%s); a group's films are merged in one format" % modes)
        layers = [int(r.get_option("film_layers")) if hasattr(lib(), "lmc_film_layer_info") else 0 for r in self.rens]
        if len(set(layers)) > 1:
            raise RuntimeError("Group: the members differ in film_layers (%s); a group's films are merged layer by layer" % layers)

    def film_overflow(self):
        """film_overflow() of the members summed (after film_reduce(): still each member's own count)"""
        return sum(r.film_overflow() for r in self.rens)

    def init_chains(self, num_init, n_chains_total, init_threads, per_chain, extra=0):
        L = lib()
        self._check_film_modes()
        L.lmc_group_chains_init.argtypes = [vp, ctypes.c_int, c_ll, ctypes.c_int, ctypes.c_int, c_ll, c_ll]
        if L.lmc_group_chains_init(self._arr, len(self.rens), num_init, n_chains_total, init_threads, per_chain, extra) != 0:
            raise RuntimeError("lmc_group_chains_init failed: " + _err())
        from . import sharding

        for ren, (b, e) in zip(self.rens, sharding.group_ranges(n_chains_total, len(self.rens))):
            ren.num_chains, ren.num_chains_total = e - b, n_chains_total
            nn, nc = ctypes.c_float(), c_ll()
            L.lmc_init_result(ren.h, ctypes.byref(nn), ctypes.byref(nc))
            ren.normalization = nn.value
        return self.rens[0].normalization, nc.value

    def step(self, n):
        L = lib()
        L.lmc_group_chains_step.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        if L.lmc_group_chains_step(self._arr, len(self.rens), n) != 0:
            raise RuntimeError("lmc_group_chains_step failed: " + _err())

    def save_checkpoint(self, path):
        """One file for the whole job: the members' chains in chain order, the job-wide state once, the members' films, counters and weight sums summed.
        Save before film_reduce()."""
        if lib().lmc_group_checkpoint_save(self._arr, len(self.rens), os.fsencode(path)) != 0:
            raise RuntimeError("lmc_group_checkpoint_save failed: " + _err())

    def load_checkpoint(self, path):
        """Takes the place of init_chains: the file's chains split over the members like init_chains splits them, whatever wrote the file (a Renderer,
        a Group of another size).  Member 0 receives the film, the counters and the weight sum.  Returns the normalization."""
        L = lib()
        self._check_film_modes()
        if L.lmc_group_checkpoint_load(self._arr, len(self.rens), os.fsencode(path)) != 0:
            raise RuntimeError("lmc_group_checkpoint_load failed: " + _err())
        from . import sharding

        total = checkpoint_info(path)["n_chains_total"]
        for ren, (b, e) in zip(self.rens, sharding.group_ranges(total, len(self.rens))):
            ren.num_chains, ren.num_chains_total = e - b, total
            nn = ctypes.c_float()
            L.lmc_init_result(ren.h, ctypes.byref(nn), None)
            ren.normalization = nn.value
        return self.rens[0].normalization

    def resident_stats(self):
        """resident_stats() of the members combined: launches, chain-steps, kernel ms and guard summed; lock steps and K of member 0 (equal on all)"""
        st = [r.resident_stats() for r in self.rens]
        out = {k: sum(d[k] for d in st) for k in ("launches", "chain_steps", "kernel_ms", "guard")}
        out.update(lock_steps=st[0]["lock_steps"], k=st[0]["k"], members=st)
        return out

    def info(self):
        """distinct devices, ordered device pairs, pairs with direct peer access enabled, host threads driving the steps"""
        o = (c_ll * 4)()
        if lib().lmc_group_info(self._arr, len(self.rens), o) != 0:
            raise RuntimeError(_err())
        return dict(devices=o[0], peer_pairs=o[1], peer_pairs_enabled=o[2], host_threads=o[3])

    def mc_render(self, spp, streams=None):
        """The mc integrator sharded over the members (lmc_group_mc_render): the stream range split into len(members) contiguous shards rendered
        concurrently, member 0's mc film left as their sum in member order (its mc_stats / mc_overflow / mc_coverage are the whole's), the other
        members' mc films cleared.  Members that differ in "mc_film_exact" are refused before anything is rendered.  Returns member 0's film."""
        begin, end = (0, -1) if streams is None else (int(streams[0]), int(streams[1]))
        if lib().lmc_group_mc_render(self._arr, len(self.rens), int(spp), begin, end) != 0:
            raise RuntimeError("lmc_group_mc_render failed: " + _err())
        return self.rens[0].mc_film()

    def mc_accumulate(self, spp, streams=None):
        """... the same range added to the exact film member 0 already holds (lmc_group_mc_accumulate)"""
        begin, end = (0, -1) if streams is None else (int(streams[0]), int(streams[1]))
        if lib().lmc_group_mc_accumulate(self._arr, len(self.rens), int(spp), begin, end) != 0:
            raise RuntimeError("lmc_group_mc_accumulate failed: " + _err())
        return self.rens[0].mc_film()

    def film_reduce(self):
        """Every member's device film becomes the sum over the members (peer copies: the in-process lmc_film_allreduce); returns its wall time in ms."""
        L = lib()
        L.lmc_group_film_reduce.argtypes = [vp, ctypes.c_int, vp]
        ms = ctypes.c_double()
        if L.lmc_group_film_reduce(self._arr, len(self.rens), ctypes.byref(ms)) != 0:
            raise RuntimeError("lmc_group_film_reduce failed: " + _err())
        return ms.value


ROW_WORDS = 48  # include/lmc_abi.h LMC_ROW_WORDS
TRACE_MAGIC = b"LMCTRACE"


def trace_file_read(path):
    """A trace file of `dpt_amd --trace-file` (little-endian: "LMCTRACE", u32 version 1, u32 row words, u32 n, u32 steps, i64 first step, n x i32
    chain ids, steps x n x row-words float32) -> dict(ids, first_step, rows[steps, n, row_words])"""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 32 or data[:8] != TRACE_MAGIC:
        raise ValueError("%s: not a chain trace file (magic)" % path)
    version, words, n, steps = (int(v) for v in np.frombuffer(data, "<u4", 4, 8))
    if version != 1:
        raise ValueError("%s: chain trace version %d, this reader knows 1" % (path, version))
    first = int(np.frombuffer(data, "<i8", 1, 24)[0])
    need = 32 + 4 * n + 4 * steps * n * words
    if len(data) != need:
        raise ValueError("%s: %d bytes, the header asks for %d" % (path, len(data), need))
    ids = np.frombuffer(data, "<i4", n, 32).astype(np.int32)
    rows = np.frombuffer(data, "<f4", steps * n * words, 32 + 4 * n).astype(np.float32).reshape(steps, n, words)
    return dict(ids=ids, first_step=first, rows=rows)


def device_count():
    """HIP devices visible to this process (0 without a GPU)."""
    return int(lib().lmc_device_count())


def checkpoint_info(path):
    """The header of a checkpoint file as a dict (host only): fingerprint fields, n_chains_total, samples_per_chain, steps_done, wall_seconds, sizes."""
    import json

    buf = ctypes.create_string_buffer(4096)
    n = lib().lmc_checkpoint_info(os.fsencode(path), buf, len(buf))
    if n < 0:
        raise RuntimeError("lmc_checkpoint_info failed: " + _err())
    return json.loads(buf.value.decode())


def mc_file_info(path):
    """The header of an mc film state file (Renderer.mc_save) as a dict (host only): fingerprint fields, n_tiles, spp (the divisor), paths, contributions,
    overflow, coverage (a list of [begin, end]), film_words, words_offset, total_bytes."""
    import json

    buf = ctypes.create_string_buffer(1 << 16)
    n = lib().lmc_mc_file_info(os.fsencode(path), buf, len(buf))
    if n < 0:
        raise RuntimeError("lmc_mc_file_info failed: " + _err())
    return json.loads(buf.value.decode())


def mc_file_words(path):
    """The film words of an mc film state file, int64 [H, W, 3], read here from the file's bytes (little-endian; layout in include/lmc_abi.h): 96 fixed
    bytes with the number of coverage ranges R at byte 12 and width, height at bytes 28 and 32, then R x 16 bytes of ranges, then the words."""
    raw = open(path, "rb").read()
    if len(raw) < 96 or raw[:8] != b"LMCMCFX\n":
        raise RuntimeError("mc_file_words: %s is not an mc film state file" % path)
    n_ranges = int(np.frombuffer(raw, "<u4", 1, 12)[0])
    width, height = (int(v) for v in np.frombuffer(raw, "<i4", 2, 28))
    at, n = 96 + 16 * n_ranges, width * height * 3
    if len(raw) != at + 8 * n:
        raise RuntimeError("mc_file_words: %s has %d bytes, its header asks for %d" % (path, len(raw), at + 8 * n))
    return np.frombuffer(raw, "<i8", n, at).astype(np.int64).reshape(height, width, 3)


def mc_coverage_probe(adds, total):
    """Test probe of the coverage arithmetic (host only): the (begin, end) ranges added in turn to an empty coverage ->
    (accepted flags, ranges held, complement within [0, total))"""
    a = np.ascontiguousarray(adds, np.int64).reshape(-1, 2)
    cap = len(a) + 2
    acc = np.zeros(max(len(a), 1), np.int32)
    cov, comp = np.zeros((cap, 2), np.int64), np.zeros((cap, 2), np.int64)
    nc, nm = ctypes.c_int(), ctypes.c_int()
    if lib().lmc_mc_coverage_probe(P(a), len(a), int(total), P(acc), P(cov), cap, ctypes.byref(nc), P(comp), cap, ctypes.byref(nm)) != 0:
        raise RuntimeError("lmc_mc_coverage_probe failed")
    return ([bool(v) for v in acc[: len(a)]], [tuple(int(v) for v in r) for r in cov[: nc.value]], [tuple(int(v) for v in r) for r in comp[: nm.value]])


def mc_chunks_probe(begin, end, n_tiles, launch_streams):
    """Test probe (host only): the launches a render call over [begin, end) is cut into, as (begin, end) pairs"""
    n = lib().lmc_mc_chunks_probe(int(begin), int(end), int(n_tiles), int(launch_streams), None, 0)
    o = np.zeros((max(n, 1), 2), np.int64)
    lib().lmc_mc_chunks_probe(int(begin), int(end), int(n_tiles), int(launch_streams), P(o), n)
    return [tuple(int(v) for v in r) for r in o[:n]]


def film_layer_splat_probe(width, height, mode, max_depth, screen_xy, rgb, cl):
    """Test probe: the splats (screen_xy [n, 2], rgb [n, 3], techniques cl [n, 2] = camDepth, lightDepth) through the device's layered splat routine
    into a fresh film.  Returns (words int64 [n_layers, H, W, 3], overflow word, splats outside the table)."""
    xy = np.ascontiguousarray(screen_xy, np.float32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(cl, np.int32).reshape(-1, 2)
    if not (len(xy) == len(c) == len(t)):
        raise ValueError("film_layer_splat_probe: screen_xy, rgb and cl differ in length")
    n_layers = film_layer_count(mode, max_depth)
    out = np.zeros((max(n_layers, 1), height, width, 3), np.int64)
    ovf, outside = c_ll(), c_ll()
    if lib().lmc_film_layer_splat_probe(width, height, mode, max_depth, len(xy), P(xy), P(c), P(t), P(out), ctypes.byref(ovf), ctypes.byref(outside)) != 0:
        raise RuntimeError("lmc_film_layer_splat_probe failed: " + _err())
    return out[:n_layers], int(ovf.value), int(outside.value)


def film_splat_probe(width, height, screen_xy, rgb, exact=True):
    """Test probe: the splats (screen_xy [n, 2] in [0, 1)^2, rgb [n, 3]) through the device's splat routine into a fresh film, one launch of n lanes in
    64-thread blocks.  exact: returns (words int64 [H, W, 3], float view [H, W, 3], overflow count); else (None, float film, 0)."""
    xy = np.ascontiguousarray(screen_xy, np.float32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    if len(xy) != len(c):
        raise ValueError("film_splat_probe: screen_xy and rgb differ in length")
    fx = np.zeros((height, width, 3), np.int64) if exact else None
    fl = np.zeros((height, width, 3), np.float32)
    ov = c_ll()
    if lib().lmc_film_splat_probe(int(width), int(height), len(xy), P(xy), P(c), 1 if exact else 0, P(fx) if exact else None, P(fl), ctypes.byref(ov)) != 0:
        raise RuntimeError("lmc_film_splat_probe failed: " + _err())
    return fx, fl, int(ov.value)


# ---- test probes of the bookkeeping launches (include/lmc_abi.h; references in tests/list_cases.py).  Integer arrays in, integer arrays out.
PROBE_SENTINEL = -0x5A5A5A5B  # what a probe's output holds where the launch wrote nothing
PROBE_BINS = 336
PROBE_CACHE_ROWS = 3000
PROBE_UNTOUCHED_BITS = 0x7FC0BEEF  # ... and a float output: a NaN with this bit pattern


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _probe(name, r):
    if r != 0:
        raise RuntimeError("%s failed: %s" % (name, _err()))


def scan_probe(values):
    """LaunchInclusiveScan on int32 values (at least one): the inclusive prefix sums, int32"""
    v = _i32(values)
    out = np.full(len(v), PROBE_SENTINEL, np.int32)
    _probe("lmc_scan_probe", lib().lmc_scan_probe(len(v), P(v), P(out)))
    return out


def radix_sort_probe(keys, n=None):
    """LaunchRadixSort24 on the first n of the len(keys) 24-bit keys (n lives in device memory): (vals, sorted keys), both len(keys) long"""
    k = np.ascontiguousarray(keys, np.uint32)
    n = len(k) if n is None else int(n)
    vals, out = np.zeros(len(k), np.int32), np.zeros(len(k), np.uint32)
    _probe("lmc_radix_sort_probe", lib().lmc_radix_sort_probe(n, len(k), P(k), P(vals), P(out)))
    return vals, out


def sort_by_technique_probe(next_kind, entries, max_entries):
    """LaunchSortByTechnique: the list's entries grouped by next_kind[chain] >> 2; the probe itself checks that nothing beyond the count is written"""
    nk, e = np.ascontiguousarray(next_kind, np.uint8), _i32(entries)
    out = np.full(len(e), PROBE_SENTINEL, np.int32)
    _probe("lmc_sort_by_technique_probe", lib().lmc_sort_by_technique_probe(len(nk), P(nk), len(e), P(e), int(max_entries), P(out)))
    return out


def build_lists_probe(next_kind, sort_plain, lean_dims=0, want_step_kind=True):
    """LaunchBuildLists: dict(large, generic, plain: N entries each, the sentinel beyond the count; counts[3]; step_kind[N] or None)"""
    nk = np.ascontiguousarray(next_kind, np.uint8)
    n = len(nk)
    o = dict(large=np.zeros(n, np.int32), generic=np.zeros(n, np.int32), plain=np.zeros(n, np.int32), counts=np.zeros(3, np.int32),
             step_kind=np.zeros(n, np.uint8) if want_step_kind else None)
    _probe("lmc_build_lists_probe", lib().lmc_build_lists_probe(n, P(nk), int(sort_plain), int(lean_dims) & 0xFFFFFFFF, 1 if want_step_kind else 0, P(o["large"]),
                                                              P(o["generic"]), P(o["plain"]), P(o["counts"]), P(o["step_kind"]) if want_step_kind else None))
    return o


def bins_compact_probe(bin_of, count, entries, grid_blocks):
    """LaunchBinsCompact: (items[N], start[PROBE_BINS])"""
    b, c, e = _i32(bin_of), _i32(count), _i32(entries)
    if len(c) != PROBE_BINS:
        raise ValueError("bins_compact_probe: count has %d entries, not %d" % (len(c), PROBE_BINS))
    items, start = np.zeros(len(b), np.int32), np.zeros(PROBE_BINS, np.int32)
    _probe("lmc_bins_compact_probe", lib().lmc_bins_compact_probe(len(b), P(b), P(c), len(e), P(e), int(grid_blocks), P(items), P(start)))
    return items, start


def split_list_probe(entries, parts, stride, grid_blocks):
    """LaunchSplitList: (sub[parts, stride], sub_count[parts])"""
    e = _i32(entries)
    sub, cnt = np.zeros((parts, stride), np.int32), np.zeros(parts, np.int32)
    _probe("lmc_split_list_probe", lib().lmc_split_list_probe(len(e), P(e), int(parts), int(stride), int(grid_blocks), P(sub), P(cnt)))
    return sub, cnt


def cache_push_probe(push_dim, push_data, slot_of, initial_counts):
    """LaunchCachePush: push_dim[N] and push_data[N, 37] (pss 12 | v1 12 | v2 12 | weight) by slot, slot_of[N] or None ->
    (rows float32 [4 dims, 3 arrays, PROBE_CACHE_ROWS, 12], weights [4, PROBE_CACHE_ROWS], counts[4], push_dim afterwards)"""
    d, x, c0 = _i32(push_dim), np.ascontiguousarray(push_data, np.float32), _i32(initial_counts)
    if x.shape != (len(d), 37) or len(c0) != 4:
        raise ValueError("cache_push_probe: push_data must be N x 37, initial_counts 4 long")
    so = None if slot_of is None else _i32(slot_of)
    rows, w = np.zeros((4, 3, PROBE_CACHE_ROWS, 12), np.float32), np.zeros((4, PROBE_CACHE_ROWS), np.float32)
    counts, after = np.zeros(4, np.int32), np.zeros(len(d), np.int32)
    _probe("lmc_cache_push_probe", lib().lmc_cache_push_probe(len(d), P(d), P(x), None if so is None else P(so), P(c0), P(rows), P(w), P(counts), P(after)))
    return rows, w, counts, after


def reloc_plan_probe(step_kind, c, l, flags, placed_key, without_gaussian_only, capacity, skipped_before):
    """LaunchRelocPlan: (count[2], members[N], sorted[N])"""
    sk, c, l, f, pk = np.ascontiguousarray(step_kind, np.uint8), _i32(c), _i32(l), _i32(flags), np.ascontiguousarray(placed_key, np.uint32)
    n = len(sk)
    count, members, srt = np.zeros(2, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _probe("lmc_reloc_plan_probe", lib().lmc_reloc_plan_probe(n, P(sk), P(c), P(l), P(f), P(pk), 1 if without_gaussian_only else 0, int(capacity), int(skipped_before),
                                                            P(count), P(members), P(srt)))
    return count, members, srt


# ---- test probes of the wave-cooperative derivative launches on a caller-given work list (include/lmc_abi.h; cases in tests/coop_cases.py).  Outputs are
# float32 arrays pre-filled with PROBE_UNTOUCHED_BITS: view them as uint32 to see which rows a launch wrote.
PROBE_VERT_WORDS = 592
COOP_KERNELS = ("mala_grad", "h2_hess", "h2_gauss")  # the `kernel` argument of coop_plan_probe, by index


def _work_list(items, count, start):
    it, cnt, st = _i32(items), _i32(count), _i32(start)
    if len(cnt) != PROBE_BINS or len(st) != PROBE_BINS:
        raise ValueError("work list: count and start must have %d entries" % PROBE_BINS)
    return it, cnt, st


def _record_list_probe(name, row_words, primary, c, l, vert, scene38, items, count, start, grid_blocks):
    pr, ve, sc = np.ascontiguousarray(primary, np.float32), np.ascontiguousarray(vert, np.float32), np.ascontiguousarray(scene38, np.float32)
    c, l = _i32(c), _i32(l)
    n = len(c)
    if pr.shape != (n, 17) or ve.shape != (n, PROBE_VERT_WORDS) or len(l) != n or sc.shape != (38,):
        raise ValueError("%s: primary must be N x 17, vert N x %d, c and l N long, scene38 38 long" % (name, PROBE_VERT_WORDS))
    it, cnt, st = _work_list(items, count, start)
    out = np.zeros((n, row_words), np.float32)
    _probe(name, getattr(lib(), name)(n, P(pr), P(c), P(l), P(ve), P(sc), len(it), P(it), P(cnt), P(st), int(grid_blocks), P(out)))
    return out


def mala_grad_list_probe(primary, c, l, vert, scene38, items, count, start, grid_blocks):
    """k_mala_grad over the work list (items, count[PROBE_BINS], start[PROBE_BINS]) of N states: rows [N, 32] = gradient (dim words) | .. | logLum at 16"""
    return _record_list_probe("lmc_mala_grad_list_probe", 32, primary, c, l, vert, scene38, items, count, start, grid_blocks)


def h2_hess_list_probe(primary, c, l, vert, scene38, items, count, start, grid_blocks):
    """k_h2_hess over the work list of N states: rows [N, 288] = gradient | logLum at 16 | Hessian rows from 32 (stride dim)"""
    return _record_list_probe("lmc_h2_hess_list_probe", 288, primary, c, l, vert, scene38, items, count, start, grid_blocks)


def h2_gauss_list_probe(dim, grad, hess, flags, offset, stage, sigma, items, count, start, grid_blocks):
    """k_h2_gauss over the work list of N chains (dim[N], grad [N, 16], hess [N, 256] at stride dim, flags[N], offset [N, 16]):
    (gauss [2, N, 544] = both buffers, px [N])"""
    d, f = _i32(dim), _i32(flags)
    n = len(d)
    g, h, o = np.ascontiguousarray(grad, np.float32), np.ascontiguousarray(hess, np.float32), np.ascontiguousarray(offset, np.float32)
    if g.shape != (n, 16) or h.shape != (n, 256) or o.shape != (n, 16) or len(f) != n:
        raise ValueError("h2_gauss_list_probe: grad and offset must be N x 16, hess N x 256, dim and flags N long")
    it, cnt, st = _work_list(items, count, start)
    gauss, px = np.zeros((2, n, 544), np.float32), np.zeros(n, np.float32)
    _probe("lmc_h2_gauss_list_probe", lib().lmc_h2_gauss_list_probe(n, P(d), P(g), P(h), P(f), P(o), int(stage), float(sigma), len(it), P(it), P(cnt), P(st),
                                                                  int(grid_blocks), P(gauss), P(px)))
    return gauss, px


def coop_plan_probe(kernel, tech):
    """No device: (states per task, record words a wave stages per state) of COOP_KERNELS[kernel] for the technique index tech"""
    a, b = ctypes.c_int(), ctypes.c_int()
    _probe("lmc_coop_plan_probe", lib().lmc_coop_plan_probe(int(kernel), int(tech), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


# ---- test probe of the texture look-up and the BSDFs (include/lmc_abi.h lmc_shade_probe; cases and references in tests/shade_cases.py, tests/shade_ref.py)
SHADE_OPS = ("tex", "evaluate", "sample")  # the `op` argument of shade_probe, by index
SHADE_MAT_WORDS, SHADE_INT_WORDS, SHADE_IN_WORDS, SHADE_OUT_WORDS = 29, 3, 20, 9


def shade_probe_args(materials, bitmap_wh, bitmap_gamma, texels, case_ints, case_in):
    """The arrays of lmc_shade_probe, contiguous and typed as the C call reads them (shared with the host build of the same source in tests/)"""
    m = np.ascontiguousarray(materials, np.float32)
    wh, ga, tx = _i32(bitmap_wh).reshape(-1, 2), np.ascontiguousarray(bitmap_gamma, np.float32), np.ascontiguousarray(texels, np.float32).ravel()
    ci, cin = _i32(case_ints), np.ascontiguousarray(case_in, np.float32)
    if m.ndim != 2 or m.shape[1] != SHADE_MAT_WORDS or len(ga) != len(wh) or ci.shape != (len(cin), SHADE_INT_WORDS) or cin.shape[1:] != (SHADE_IN_WORDS,):
        raise ValueError("shade_probe: materials must be n_mat x %d, bitmap_wh n_bitmaps x 2, bitmap_gamma n_bitmaps, case_ints n x %d, case_in n x %d"
                         % (SHADE_MAT_WORDS, SHADE_INT_WORDS, SHADE_IN_WORDS))
    return m, wh, ga, tx, ci, cin


def shade_probe(op, glossy, materials, bitmap_wh, bitmap_gamma, texels, case_ints, case_in, n=None, n_rows=None):
    """EvalTex (op 0), BsdfEvaluate<glossy> (1) or BsdfSample<glossy> (2) of device/dshade.h, one case per lane, on the first n cases:
    (ok int32 [n_rows], out float32 [n_rows, 9] = wo | contrib | cosWo | pdf | revPdf); rows from n on keep PROBE_SENTINEL / PROBE_UNTOUCHED_BITS"""
    m, wh, ga, tx, ci, cin = shade_probe_args(materials, bitmap_wh, bitmap_gamma, texels, case_ints, case_in)
    n = len(cin) if n is None else int(n)
    n_rows = n if n_rows is None else int(n_rows)
    if n > len(cin):
        raise ValueError("shade_probe: n exceeds the cases given")
    ok, out = np.zeros(max(n_rows, 1), np.int32), np.zeros((max(n_rows, 1), SHADE_OUT_WORDS), np.float32)
    _probe("lmc_shade_probe", lib().lmc_shade_probe(int(op), int(glossy), len(m), P(m), len(wh), P(wh), P(ga), P(tx), len(tx), n, n_rows, P(ci), P(cin), P(ok), P(out)))
    return ok, out


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it, the host program broadcasts it)"""
    buf = (ctypes.c_ubyte * 128)()
    if lib().lmc_comm_unique_id(buf) != 0:
        raise RuntimeError("lmc_comm_unique_id failed: " + _err())
    return bytes(buf)


def read_image(path):
    """EXR / PNG -> float32 [H, W, 3] through the library's own readers."""
    w, h = ctypes.c_int(), ctypes.c_int()
    if lib().lmc_image_read(path.encode(), ctypes.byref(w), ctypes.byref(h), None) != 0:
        raise RuntimeError(_err())
    out = np.zeros((h.value, w.value, 3), np.float32)
    if lib().lmc_image_read(path.encode(), None, None, P(out)) != 0:
        raise RuntimeError(_err())
    return out


def write_exr(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    if lib().lmc_image_write_exr(path.encode(), P(rgb), rgb.shape[1], rgb.shape[0]) != 0:
        raise RuntimeError(_err())


def grad_batch(c, l, primary_soa, scene38, vert_soa, want_grad=True):
    """n evaluations of the (c,l) path program on the GPU; SoA word-major inputs (see include/lmc_abi.h)."""
    primary_soa = np.ascontiguousarray(primary_soa, np.float32)
    vert_soa = np.ascontiguousarray(vert_soa, np.float32)
    scene38 = np.ascontiguousarray(scene38, np.float32)
    n = primary_soa.shape[1]
    L = max(c + l - 1, 2)
    ll = np.zeros(n, np.float32)
    g = np.zeros((2 * L, n), np.float32)
    r = lib().lmc_grad_batch(c, l, n, P(primary_soa), P(scene38), P(vert_soa), P(ll), P(g) if want_grad else None)
    if r != 0:
        raise RuntimeError("lmc_grad_batch failed: " + _err())
    return ll, g


def smoke():
    """One small invocation of the hot path on cuda:0, checked against the CPU oracle (test infrastructure)."""
    import sys

    sys.path.insert(0, ROOT)
    from tests import gpu_checks

    gpu_checks.smoke()
