/* lmc_abi.h -- C ABI of the MI355X (gfx950) back end for the Langevin-MCMC chain loop.
 *
 * Drop-in boundary.  Two groups of entry points, all `extern "C"`, plain pointers and sizes:
 *
 * (1) The reference's own in-process plugin ABI: the shared object it dlopen()s as
 *     $DPT_LIBPATH/pathlibbidir_mala.so and resolves by name with dlsym
 *     (/root/reference/src/chad.cpp:884-895,1000-1016; names path.cpp:3404-3417; loop path.cpp:4028-4057):
 *         void evaluate_path_bidir_mala_<c>_<l>_static     (lens[2], primary[2L+1], scene[38], vertParams[V], logLum[1])
 *         void evaluate_path_bidir_mala_<c>_<l>_static_derv(lens[2], primary[2L+1], scene[38], vertParams[V], grad[2L])
 *     for 1<=c<=9, 0<=l<=8, 3<=c+l<=9 (L = c+l-1, V = 238+59(c+l-3)).  Caller type: PathFunc / PathFuncDerv
 *     (/root/reference/src/path.h:121-125); the caller passes a 6th NULL `hess` argument in MALA mode
 *     (mutation_mala.h:102-107), which these symbols ignore.  Each call launches the HIP kernel on one path;
 *     lmc_grad_batch is the entry point meant for throughput.
 *
 * (2) The batched / resident interface that replaces the per-chain loop of MLT() (mlt.cpp:20-214): scene
 *     load (ParseScene, parsescene.cpp:627-639), MLTInit (mlt.h:41-154), the chain loop (mlt.cpp:60-196),
 *     film read-back (mlt.cpp:203-207).
 *
 * Error convention: functions returning int give 0 on success, a negative value on failure with the message
 * available from lmc_last_error(); nothing throws across the boundary.  All functions fail (never fall back
 * to a CPU path) when no HIP device is usable.
 */
#ifndef LMC_ABI_H
#define LMC_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lmc_ctx lmc_ctx;

/* Scene description: the reference's command line + <dpt> overrides (main.cpp:49-64, parsescene.cpp:535-590).
 * Integer fields <= 0 (seed_offset < 0) keep the value from the XML. */
typedef struct lmc_scene_desc {
    const char *scene_xml;  /* path of the Mitsuba-0.5-subset scene file, as given to `dpt` */
    int force_diffuse;      /* BASELINE.json config 2: every BSDF becomes `diffuse` */
    int max_depth;          /* <dpt maxdepth> override */
    int width, height;      /* film size override */
    int seed_offset;        /* --seedoffset (main.cpp:57-58) */
    int device;             /* HIP device ordinal */
    int use_gradient;       /* 1: evaluate d log f / d pss in-kernel (derivative library present);
                               0: behave like a missing pathlibbidir_mala.so (isotropic proposals, path.cpp:4042-4053) */
} lmc_scene_desc;

const char *lmc_last_error(void);

lmc_ctx *lmc_create(const lmc_scene_desc *desc);
void lmc_destroy(lmc_ctx *ctx);
/* number of HIP devices visible to this process (0 without a GPU): `device` of lmc_scene_desc must be below it */
int lmc_device_count(void);

/* Host-only (no GPU needed): what the front end parsed from a scene file (parsescene.cpp:535-639, loadserialized.cpp:153-325, parseobj.cpp:57-275,
 * image.cpp) as one JSON document: per mesh triangle / vertex counts, bounds, area, material, emitter; per material type and parameters
 * (textures: file, size, gamma, average); lights with their sampling weights and the light-pick CDF; camera; <dpt> options; output name.
 * Writes at most cap - 1 characters + NUL; returns the document's full length, -1 on error.  The cross-check surface of the parsers. */
long long lmc_scene_dump(const char *scene_xml, int force_diffuse, char *out, long long cap);
/* [width, height, numTriangles, maxDepth, numBvhNodes, bvhDepth, numLights, mala] */
int lmc_info(lmc_ctx *ctx, int *out8);
/* the 38-float scene block of the plugin ABI (scene.cpp:160-169) */
int lmc_scene_params(lmc_ctx *ctx, float *out38);
/* <dpt> float options by XML name: largestepprob, largestepscale, mala, uniformmixprob, mala-stepsize, mala-gn,
 * perturbstddev, mindepth, h2mc, uselightcoordinatesampling, largestepmultiplexed, samplecache (parsescene.cpp:538-585).  mala / h2mc /
 * samplecache / uselightcoordinatesampling select what the resident chain state and the launch plan are laid out for: the call itself succeeds
 * at any time, but once one of them differs from its value at lmc_chains_init, lmc_chains_step returns -1 until the chains are initialised again.
 * Back-end switches (no counterpart in the reference): "timing" (per-step HIP events for lmc_step_timing), "overlap" (side streams on / off),
 * "max-derivatives-depth" (main.cpp:59-60), "resort_every" / "resort_first" (period and first step of the full re-sort of the resident chains by
 * technique and screen position, device/relocate.hip; default 32 / 4, 0 = off; read at the next lmc_chains_init), "exp_resort" (measurement hook),
 * "bidirectional" (the generator of lmc_mc_render) */
int lmc_set_option(lmc_ctx *ctx, const char *name, double value);
/* <dpt> options as parsed: spp, numinitsamples, numchains, directspp, mindepth, maxdepth, largestepprob, largestepscale,
 * mala, h2mc, seedoffset (dptoptions.h:7-34); back-end state: bvh_quantised (the scene's hot launches walk the 64-byte quantised BVH nodes),
 * bvh_thick_flat_share (the figure that choice is made by); integrator_mc (1 when <string integrator> is "mc"), bidirectional (the <dpt> value,
 * which lmc_set_option "bidirectional" overrides) */
int lmc_get_option(lmc_ctx *ctx, const char *name, double *value);
/* film "filename" of the scene (outputName); the reference appends "_timeuse_<seconds>s.exr" (mlt.cpp:208) */
const char *lmc_output_name(lmc_ctx *ctx);
/* image files through the library's own codecs: EXR / PNG in (rgb == NULL: size only), RGB half ZIP EXR out (image.cpp:44-62) */
int lmc_image_read(const char *path, int *w, int *h, float *rgb);
int lmc_image_write_exr(const char *path, const float *rgb, int w, int h);

/* MLTInit (mlt.h:41-154) + chain set-up (mlt.cpp:60-90).  `init_threads` plays NumSystemCores(): init stream t is
 * seeded RNG(t + seedOffset) (mlt.h:67).  The chains [chain_begin, chain_end) of the n_chains_total chains live on
 * this device (multi-GPU: one range per rank; seeds are global chain ids, mlt.cpp:61-62).
 * samples_per_chain / chains_need_extra as computed at mlt.cpp:36-40. */
int lmc_chains_init(lmc_ctx *ctx, long long num_init_samples, int n_chains_total, int init_threads, int chain_begin, int chain_end,
                    long long samples_per_chain, long long chains_need_extra);
/* Multi-rank jobs: MLTInit is sharded by init stream (rank r runs streams [V r / R, V (r + 1) / R), V = init_threads) and the ranks
 * exchange what the seeding needs (contribution counts, scores, the checkpoints of the seeding samples), so that normalization and
 * every chain's init state equal the one-rank result bit for bit.  Ranks of an RCCL job (lmc_comm_init BEFORE lmc_chains_init) call
 * lmc_chains_init collectively; the n contexts of an in-process group (one per GPU, or several on one GPU for bring-up) are driven
 * by the two calls below (chains split into n contiguous equal ranges; their collectives are device copies). */
int lmc_group_chains_init(lmc_ctx **ctxs, int n, long long num_init_samples, int n_chains_total, int init_threads, long long samples_per_chain,
                          long long chains_need_extra);
int lmc_group_chains_step(lmc_ctx **ctxs, int n, int n_steps);
/* The film merge of such a group (the reference merges its per-thread films in-process, mlt.cpp:203-207): every member's device film (and
 * splat-weight sum) becomes the sum over the members, through peer copies -- lmc_film_allreduce without a communicator.  Once per stepped
 * film, like it.  *ms (may be NULL): wall time of the merge. */
int lmc_group_film_reduce(lmc_ctx **ctxs, int n, double *ms);
/* out4 = [distinct devices among the members, ordered pairs of distinct member devices, of which with direct peer access enabled
 * (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess, once, when the group is set up), host threads that drive the group's steps (one per
 * member; LMC_GROUP_THREADS=0: one for all)] */
int lmc_group_info(lmc_ctx **ctxs, int n, long long *out4);
/* host wall time (ms) this context's steps took to QUEUE (launches, event operations, the exchange's copies) since the last call, and the
 * number of steps: what a rank-step costs the host thread that drives it, to be read next to the step's GPU time */
int lmc_host_issue_timing(lmc_ctx *ctx, double *ms, long long *steps);
/* CPU test hooks (need no GPU): the host-side plan of the sharded MLTInit from the padded blocks the ranks all-gather.
 * lmc_shard_layout: out5 = [first stream, end stream, first sample, end sample, samples of the largest rank] of `rank`;
 * lmc_shard_counts_probe: rank_first[world + 1] = first contribution of every rank's block (and the total);
 * lmc_shard_plan_probe: per chain of the job the init sample that seeds it, the seeding contribution's technique (c * 16 + l) and
 * lsScore; owned_begin[world + 1]: rank r's samples seed the chains [owned_begin[r], owned_begin[r + 1]); normalization */
int lmc_shard_layout(int world, int rank, int init_threads, long long num_init_samples, long long *out5);
int lmc_shard_counts_probe(int world, int init_threads, long long num_init_samples, const unsigned char *padded_counts, long long max_local_samples,
                           unsigned long long *rank_first);
int lmc_shard_plan_probe(int world, int init_threads, long long num_init_samples, int n_chains_total, const unsigned char *padded_counts,
                         long long max_local_samples, const unsigned char *padded_cl, const float *padded_ls, long long max_local_contribs,
                         long long *seed_sample, unsigned char *seed_cl, float *seed_ls, int *owned_begin, float *normalization);
/* normalization = avgScore (mlt.cpp:46-47), number of init contributions */
int lmc_init_result(lmc_ctx *ctx, float *normalization, long long *num_contribs);
/* parity probe: every contribution MLTInit collected, in stream order: index of the init sample that produced it, technique as
 * c * 16 + l, lsScore; returns the total count (at most `cap` entries are written) */
long long lmc_init_contribs(lmc_ctx *ctx, long long cap, long long *sample, int *cl, float *ls);
/* advances every resident chain by n_steps mutations (the loop body mlt.cpp:91-170), lock step */
int lmc_chains_step(lmc_ctx *ctx, int n_steps);
/* blocks until all queued work is done */
int lmc_sync(lmc_ctx *ctx);
/* indirect film buffer, W*H*3 floats, un-normalised like indirectBuffer (mlt.cpp:54) */
int lmc_film_read(lmc_ctx *ctx, float *rgb);
int lmc_film_clear(lmc_ctx *ctx);
/* DirectLighting(scene, directBuffer) (direct.cpp:4-54): direct_spp samples per pixel of paths of length <= 2, tile RNG
 * streams seeded tileIndex + seedOffset; un-normalised W*H*3 buffer like directBuffer (mlt.cpp:33-34).  The image the
 * reference writes is direct / directSpp + indirect / spp (mlt.cpp:203-207). */
int lmc_direct_lighting(lmc_ctx *ctx, int direct_spp);
int lmc_direct_read(lmc_ctx *ctx, float *rgb);
/* same generator over the scene's full depth range (the reference's "mc" integrator sampler, pathtrace.cpp): an independent
 * estimator used to cross-check the MLT image; result through lmc_direct_read */
int lmc_path_trace(lmc_ctx *ctx, int spp);
/* plain Monte Carlo over GeneratePathBidir samples (path length >= 3), radiance image through lmc_direct_read: a second
 * cross-check estimator that isolates the bidirectional generator from the Markov chain */
int lmc_bidir_mc(lmc_ctx *ctx, int spp);
/* The "mc" integrator (PathTrace, pathtrace.cpp:14-78): spp samples per pixel, GeneratePathBidir with a fixed pixel when <dpt bidirectional>
 * is true, GeneratePath otherwise, over the scene's [mindepth, maxdepth]; every contribution with luminance above 1e-10 splatted with weight
 * 1 / spp into a film of its own (neither the MLT film nor the direct film; no chain state is touched).  Stream (t, s) = RNG(t + nTiles * s +
 * seedoffset), t the 16x16 tile index, s the sample index, draws sample s of every pixel of tile t; lmc_mc_render clears the MC film and
 * renders the stream ids [stream_begin, stream_end) of [0, nTiles * spp) (stream_end = -1: all), so films of disjoint ranges sum to the
 * film of their union.  With spp = 1 and seedoffset 0 the streams are the reference's own. */
int lmc_mc_render(lmc_ctx *ctx, int spp, long long stream_begin, long long stream_end);
/* the MC film, W*H*3 floats, already weighted by 1 / spp */
int lmc_mc_read(lmc_ctx *ctx, float *rgb);
/* out2[0] = paths traced, out2[1] = contributions splatted, by the last lmc_mc_render */
int lmc_mc_stats(lmc_ctx *ctx, long long *out2);
/* A render or accumulate call of either film mode runs as launches of at most lmc_set_option "mc_launch_streams" stream ids each (default 262144: a
 * 1024 x 768 render at 64 spp, 196608 ids, is one launch) on the context's stream; a cut between two launches falls on a multiple of nTiles wherever
 * one lies inside the launch it ends, and the launches' scratch is sized for one of them.  lmc_get_option "mc_launches" reports the launches of the
 * last call.  The film does not depend on the cuts (float mode: up to the order of the float adds, as between any two runs).
 *
 * Exact mc film (INTEGRATION.md "Exact mc film"): lmc_set_option "mc_film_exact" = 1 (default 0; a name of its own, "film_exact" and LMC_FILM_EXACT
 * keep governing the MLT film alone) takes effect at the next lmc_mc_render and makes the MC film W*H*3 signed 64-bit fixed-point words holding the
 * integer sum of the UNWEIGHTED contributions, so that the film is a pure function of the set of stream ids it holds: bit-equal however the ids are
 * cut into calls, launches, members or files, and from run to run.
 *   conversion   q = llrint((double)v * 4294967296.0) per component of a contribution that passed the luminance and finite tests of float mode
 *   deviations   (1) summed unweighted and divided ONCE, at read time, in double (float mode divides every contribution in float, then sums);
 *                (2) a contribution with a component |v| >= 2^30 is dropped WHOLE and counted by lmc_mc_overflow; lmc_mc_stats still counts it
 *   coverage     the film knows the stream ids it holds as disjoint, merged, ascending ranges; a range that overlaps them is refused
 *   lmc_mc_render       clears words, overflow, counters and coverage, then adds [stream_begin, stream_end) like lmc_mc_accumulate
 *   lmc_mc_accumulate   adds the ids [stream_begin, stream_end) of [0, nTiles * spp) (-1: to the end) WITHOUT clearing; spp becomes the read divisor.
 *                       Exact mode only (-1 in float mode).  An overlapping range, or a film that holds ids beyond nTiles * spp, returns -1 and
 *                       leaves film and coverage as they were.  On a context that holds no exact film yet it starts from an empty one.
 *   lmc_mc_coverage     returns the number of ranges held and writes at most cap [begin, end) pairs (0 in float mode)
 *   lmc_mc_read         converts on the device, float((double)q * 2^-32 / (double)spp), spp the divisor of the latest render / accumulate / load
 *   lmc_mc_read_fixed   the W*H*3 raw words; -1 in float mode
 *   lmc_mc_overflow     *n = contributions dropped by the range rule since the film was last cleared (0 in float mode)
 *   lmc_mc_stats        cumulative since the film was last cleared
 * lmc_group_mc_render (either mode): [stream_begin, stream_end) split at begin + (end - begin) * k / n, member k renders shard k concurrently with the
 * others (one host thread each), then member 0's film becomes the sum over the members, added in ascending member order on member 0's device (int64
 * in exact mode; float in float mode, the order a host loop over the members adds in).  Member 0's stats, overflow and coverage are the whole's, the
 * other members' MC films and counters are left cleared.  The members are distinct contexts of one scene (a device may carry several); members that
 * differ in "mc_film_exact" are refused before anything is rendered.  lmc_group_mc_accumulate (exact mode only): the same, except that member 0 adds
 * its shard to the film it holds (after lmc_mc_load, say), so it ends with what it held plus the whole range; a range that overlaps member 0's
 * coverage is refused before anything is rendered.
 * State file (exact mode only): lmc_mc_save writes path.tmp and renames it; little-endian: magic "LMCMCFX\n", uint32 version (1), uint32 R, uint64 scene hash
 * (content of the XML and the files it pulls in), int32 force_diffuse, width, height, mindepth, maxdepth, seedoffset, bidirectional, 0, int64 nTiles,
 * divisor spp, paths, contributions, overflow, R x int64 [begin, end) coverage ranges, W*H*3 int64 words.  lmc_mc_load ("mc_film_exact" = 1 on the
 * context) compares scene hash .. nTiles field by field and returns -1 naming the first that differs -- or a wrong magic, a wrong version, a short
 * file -- leaving the context as it was; after it lmc_mc_accumulate continues the render.  lmc_mc_file_info: host only, the header as JSON
 * (lmc_checkpoint_info's convention).
 * Not covered: the RCCL rank path (lmc_film_allreduce sums the MLT film only), lmc_path_trace, lmc_bidir_mc and the direct film stay float. */
int lmc_mc_accumulate(lmc_ctx *ctx, int spp, long long stream_begin, long long stream_end);
int lmc_mc_coverage(lmc_ctx *ctx, long long *ranges, int cap);
int lmc_mc_read_fixed(lmc_ctx *ctx, long long *words);
int lmc_mc_overflow(lmc_ctx *ctx, long long *n);
int lmc_group_mc_render(lmc_ctx **ctxs, int n, int spp, long long stream_begin, long long stream_end);
int lmc_group_mc_accumulate(lmc_ctx **ctxs, int n, int spp, long long stream_begin, long long stream_end);
int lmc_mc_save(lmc_ctx *ctx, const char *path);
int lmc_mc_load(lmc_ctx *ctx, const char *path);
long long lmc_mc_file_info(const char *path, char *json, long long cap);
/* Layered mc film (INTEGRATION.md "Layered mc film"): lmc_set_option "mc_layers" = 1 (by path length) or 2 (by technique), default 0 (off: the film and the
 * kernels above), takes effect at the next lmc_mc_render and, in either film mode and with either generator, renders the same streams into one film
 * per layer; the split happens where a contribution is added, so the layers of one render sum to its unlayered film -- in exact mode word for word.
 *   numbering    D = the context's maxdepth (1 .. 12), a contribution's technique (c, l) = (camDepth, lightDepth) of SubpathContrib, L = c + l - 1 its length.
 *                "mc_layers" = 1: D layers, layer L - 1 holds length L = 1 .. D.
 *                "mc_layers" = 2: D (D + 3) / 2 layers, for L = 1 .. D and l = 0 .. L (c = L + 1 - l) layer (L - 1)(L + 2) / 2 + l: 27 layers at D = 6, 44 at 8.
 *                Layers a generator or a mindepth never reaches stay zero.  A contribution outside the table cannot occur; it would be dropped (exact mode: and
 *                counted by lmc_mc_overflow), never written.
 *   storage      n_layers * W*H*3 words on the device (exact mode: int64, and one overflow word); an allocation failure names the byte count and "mc_layers"
 *   per layer    the luminance, finite and range rules, the 1 / spp weight of float mode and the counters are those of the unlayered film, per contribution;
 *                stream ranges, "mc_launch_streams" cuts and, in exact mode, lmc_mc_accumulate work as above.  lmc_mc_accumulate with "mc_layers" set to
 *                another value than the film was rendered with returns -1 and leaves the film as it was.
 *   the total    lmc_mc_read, lmc_mc_read_fixed, lmc_mc_overflow, lmc_mc_stats and lmc_mc_coverage apply to the sum of the layers (int64 adds; float mode:
 *                float adds in increasing layer index): a caller that ignores the layers sees the unlayered image, in exact mode the same words
 *   lmc_mc_layer_info        *mode, *n_layers of the film the context holds (n_layers = 0: unlayered); cl receives at most cap pairs, (L, -1) in length
 *                            mode, (c, l) in technique mode
 *   lmc_mc_read_layer        one layer as W*H*3 floats; exact mode: float((double)q * 2^-32 / (double)spp) like lmc_mc_read
 *   lmc_mc_read_layer_fixed  one layer's raw words; -1 in float mode.  A layer index outside [0, n_layers) returns -1.
 * Limits of this version: the mc integrator only (the MLT film is not layered); no state file and no group -- lmc_mc_save of a layered film, lmc_mc_load into
 * a context set to "mc_layers", lmc_group_mc_render and lmc_group_mc_accumulate with such a member return -1 naming mc_layers, render and write nothing, and
 * leave the contexts usable. */
int lmc_mc_layer_info(lmc_ctx *ctx, int *mode, int *n_layers, int *cl, int cap);
int lmc_mc_read_layer(lmc_ctx *ctx, int layer, float *rgb);
int lmc_mc_read_layer_fixed(lmc_ctx *ctx, int layer, long long *words);
/* test hooks of the host-side bookkeeping (host/mcfilm.cpp), host only.  coverage_probe: the n_adds ranges adds[2 i], adds[2 i + 1] are added in turn to an
 * empty coverage, accepted[i] = 1 / 0; cov / comp receive the ranges then held / what [0, total) lacks (at most their cap pairs; *n_cov / *n_comp the full
 * numbers).  chunks_probe: the launches a call over [begin, end) is cut into; returns their number, writes at most cap pairs. */
int lmc_mc_coverage_probe(const long long *adds, int n_adds, long long total, int *accepted, long long *cov, int cov_cap, int *n_cov, long long *comp, int comp_cap, int *n_comp);
int lmc_mc_chunks_probe(long long begin, long long end, long long n_tiles, long long launch_streams, long long *out, int cap);
/* out[0..7] = steps, largeSteps, accepted, gradCalls, cacheQueries, cacheHits, resets, cacheReadyMask; *weight_sum =
 * sum over steps of the splatted weight (film luminance == normalization * weight_sum) */
int lmc_stats(lmc_ctx *ctx, long long *out8, double *weight_sum);
/* per-chain summary, `stride` floats each (>= 32), same layout as the oracle's orc_chain_summary:
 * [valid, camDepth, lightDepth, lsScore, ssScore, scoreSum, time, gaussianInitialized, buffered, sampleIdx,
 *  screenX, screenY, contribR, contribG, contribB, nSplats, pss[0..15]]; which = 0 current, 1 init states.
 * Of an INVALID current state (valid == 0) only lsScore and the technique mean anything: the chain loop reads nothing else of it (mlt.cpp:148,
 * mutation_large.h:87-116), and after an outlier reset (mlt.cpp:151-158) onto an init state that lives on another rank of the job only those
 * are copied -- the path words (time, pss, screen) of such a row are the previous state's. */
int lmc_chain_summary(lmc_ctx *ctx, int which, float *out, int stride);
/* chain relocation (device/relocate.hip; no counterpart in the reference, whose chains are objects a thread walks, mlt.cpp:60-196): from the
 * FIRST step on -- the cache-fill phase included -- the resident chains are kept physically grouped by technique (c,l): after every step's large-step
 * launch, on its stream, the chains that launch gave another technique move to the slots of their technique (the small-step launches' chains are not
 * touched; the step's cache pushes are packed before the move, in chain order).  Invisible in every result except the order of the film's atomics;
 * lmc_chain_summary reports rows in chain order regardless.
 * out4 = [relocations run, chains moved by the last one, adjacent slot pairs whose chains differ in technique key, slots]; -1 when off */
int lmc_relocation_stats(lmc_ctx *ctx, long long *out4);
/* relocations skipped so far because their movers exceeded the staging records (N / 2 after the first full sort): such a step's movers stay where
 * they are -- a performance event only, visible here and as "chains moved by the last one" = 0; -1 when relocation is off */
long long lmc_relocation_skipped(lmc_ctx *ctx);
/* the resident schedule (lmc_set_option "resident_steps" = K >= 1; 0, the default, is lock step only; refused on H2MC contexts): once every
 * relevant gradient cache is frozen -- from the step in which the last one becomes ready, mid-call included; plain MLT from the first step --
 * lmc_chains_step / lmc_group_chains_step(n) run their remaining steps as ceil(remaining / K) launches (device/step_resident.hip) in which every
 * chain advances by up to K complete mutations on its own (no other launch, no host round trip in between), and hand back to lock step with
 * the next step's work lists built.  Same trajectories as lock step, chain for chain; the film differs only in the order of its float atomics.
 * K is capped so that one launch stays in the tens of milliseconds.  "resident_lanes" (16 / 32 / 64; 0, the default: 32 up to 2^16 chains, 64
 * above): chains per 64-lane wave.
 * lmc_get_option "resident_guard": steps of resident launches that would have needed the gradient program or a cache push (0 by construction).
 * out4 = [resident launches, chain-steps advanced by them, lock steps run, K in force] since lmc_chains_init; *kernel_ms (may be NULL): HIP-event
 * time of the resident launches */
int lmc_resident_stats(lmc_ctx *ctx, long long *out4, double *kernel_ms);
/* kernel time (ms, HIP events on the launch stream) and launch count of the chain-step kernel since the last call */
int lmc_step_timing(lmc_ctx *ctx, double *kernel_ms, long long *launches);
/* split of the interval the last lmc_step_timing call covered: out3[0] = ms inside the lean small-step kernel
 * (k_step_small, the dominant kernel), out3[1] = ms inside the large-step + generic small-step launches,
 * out3[2] = chain-steps the lean kernel has run since lmc_chains_init (cumulative). */
int lmc_kernel_timing(lmc_ctx *ctx, double *out3);
/* the same interval, the three step launches separately: out4 = [lean small-step ms, large-step ms, generic small-step ms
 * (cache-filling gradient steps; every small step of an H2MC render), cumulative chain-steps of the lean kernel] */
int lmc_kernel_timing_split(lmc_ctx *ctx, double *out4);

/* ---- multi-GPU (one process per GPU; chains sharded by contiguous global id range through lmc_chains_init).
 * The only data-path collective is the sum of the per-GPU films: rank 0 calls lmc_comm_unique_id and the host program
 * ships the 128 bytes to the other ranks (any side channel), every rank calls lmc_comm_init, and after its last step
 * lmc_film_allreduce sums the device films in place with RCCL on the step stream (no host staging) together with the
 * splat-weight sum.  lmc_film_device_ptr exposes the device buffer for hosts that bring their own collective library. */
int lmc_comm_unique_id(unsigned char *out128);
int lmc_comm_init(lmc_ctx *ctx, int n_ranks, int rank, const unsigned char *id128);
int lmc_film_allreduce(lmc_ctx *ctx);
/* Driver plumbing over the job's own communicator (no second communication library): n <= LMC_COMM_MAX_SCALARS host doubles reduced over
 * the ranks in place (op 0 sum, 1 max, 2 min), blocking; and a barrier (own stream drained, then a one-word all-reduce). */
#define LMC_COMM_MAX_SCALARS 64
int lmc_comm_allreduce_f64(lmc_ctx *ctx, double *vals, int n, int op);
int lmc_comm_barrier(lmc_ctx *ctx);
void *lmc_film_device_ptr(lmc_ctx *ctx, long long *n_floats);

/* Batched path program: n evaluations of technique (c,l); SoA, word-major: primary_soa[(2L+1)*n],
 * vert_soa[V*n], grad_soa[2L*n] (word w of item i at [w*n + i]); scene38 as lmc_scene_params.  Host pointers.
 * loglum and grad_soa may each be NULL. */
int lmc_grad_batch(int c, int l, int n, const float *primary_soa, const float *scene38, const float *vert_soa, float *loglum, float *grad_soa);

/* H2MC library (the reference's pathlibbidir.so): symbols evaluate_path_bidir_<c>_<l>_static{,_derv}, the derivative with
 * a 6th `hess` argument ((2L)^2 floats, row i at hess[i*2L]; path.h:122-123, mutation_h2mc.h:74-79), are exported next to
 * the MALA ones.  Batched form: hess_soa[(2L)^2 * n], entry (i,k) of item j at [(i*2L + k)*n + j]. */
int lmc_hess_batch(int c, int l, int n, const float *primary_soa, const float *scene38, const float *vert_soa, float *loglum, float *grad_soa, float *hess_soa);

/* Parity probe: the rows of one global-cache dim as they stand (global_cache.h:21-23 point_cloud_t).  pss: 3000 x dim, weight: 3000,
 * extra: 3000 x 313 = every row's path words then its contribution words, only with `samplecache` (mutation_large_cache.h); any
 * pointer may be NULL.  Returns the number of rows filled, -1 on error. */
int lmc_cache_rows(lmc_ctx *ctx, int dim, float *pss, float *weight, float *extra);
/* Parity probe of LargeStepCache's cache-side pieces on the device (`samplecache`, dim ready): row[i] = sampleCache with the uniform
 * u[i] (global_cache.h:126-137), pdf[i] = evalPdfCache at query[i * dim ..] for technique cl[2 i], cl[2 i + 1] (:139-164).
 * Returns 0, -2 when the dim is not ready or the option is off, -1 on error. */
int lmc_cache_probe(lmc_ctx *ctx, int dim, int n, const float *u, int *row, const float *query, const int *cl, float *pdf);

/* ---- probes used by the parity tests (tests/) ---- */
/* rays: n x [ox,oy,oz,dx,dy,dz,tnear,tfar]; closest hit -> global triangle id (or -1) and t
 * (environment LMC_TRACE_TIGHT=1, read at every call: both walks fetch a leaf's triangles two per round, as the three-wave lean launches do) */
int lmc_trace(lmc_ctx *ctx, int n, const float *rays, int *prim, float *t);
int lmc_occluded(lmc_ctx *ctx, int n, const float *rays, int *occluded);
/* mode 0 raw u32, 1 uniform01 bits, 2 one normal_distribution object, 3 mixed (u,u,7 normals per round); + 8: the extension table synthesised from
 * the seed until the stream ticks, as the chain kernels do (device/drng.h) instead of read from memory;
 * out: n_seeds x (n + 66) words, the last 66 = RNG state after the draws [lo, hi, table 64] */
int lmc_rng_probe(int n_seeds, const unsigned long long *seeds, int mode, int n, float mean, float stddev, unsigned *out);
int lmc_kd_probe(int dim, int npts, const float *pts, int nq, const float *q, float radius_sq, int knn, int *out_n, int *out_idx, float *out_dist);
/* test hook: first index of cdf[0..n) that is not below u[i] (the device's search behind the env-map CDF look-ups; = std::lower_bound) */
int lmc_lower_bound_probe(int n, const float *cdf, int nq, const float *u, int *out);
/* measurement aid: ms per launch of a kernel that streams `words` state words per chain in batches of `batch` loads; mode 0 = [word][chain], 1 = [tile of 64][word][lane] */
int lmc_layout_probe(int nChains, int words, int mode, int batch, int reps, double *msPerLaunch);
/* test hook (no device): the LDS plan of the lean small-step launch for a tree whose traversal stack needs bvh_stack_need entries: the stack words of a
 * thread (the need rounded up to 4, at least 24), its LDS words in all (+ 24), and the dynamic bytes of a block of block_threads */
int lmc_lean_plan_probe(int bvh_stack_need, int block_threads, int *stack_words, int *lds_words_per_thread, long long *lds_bytes_per_block);
/* what the context's lean small-step launch is (no launch): out16[0 .. 7] = leaves of the uploaded tree that hold 1 .. 8 triangles, [8] = the tree's stack
 * need, [9] = LDS stack words of a thread, [10 .. 14] = the instantiation of k_step_small it takes: LDS stack, glossy, without light sub-paths, quantised
 * nodes, the register-saving forms of the three-wave launches (two leaf triangles per round), [15] = threads per block */
int lmc_lean_info(lmc_ctx *ctx, int *out16);
/* parity probe, evaluated on the device: the deterministic float exp (mode 0) / log (1) / pow (2) of the glossy BSDFs (device/dtrans.h), sin (3) / cos (4) /
 * acos (5) / atan2(x, y) (6) of the sampling code (device/dtrig.h), and glibc's logf as restated for the normal distribution (7, device/drng.h) */
int lmc_trans_probe(int n, int mode, const float *x, const float *y, float *out);
/* measurement hook (LMC_PROF=1): wave cycles per region of the lean small-step kernel since the last call: out16[0 .. LMC_PROF_REGIONS-1]
 * = cycle sums of the regions (dsmall.h PR_*), out16[LMC_PROF_REGIONS] = number of waves */
#define LMC_PROF_REGIONS 15
int lmc_prof_read(lmc_ctx *ctx, unsigned long long *out16);
/* test hook: compares the device-built existence-test grid of one cache dim with the host build; number of differing cells (0 = same), -2 = that cache is not ready */
int lmc_cache_grid_check(lmc_ctx *ctx, int dim);
/* the lean kernel's existence test in front of the cache query, evaluated on the host: out[i] = 1 iff a cache point lies within the radius */
int lmc_cache_filter_probe(int dim, int npts, const float *pts, int nq, const float *q, int *out);
/* test probe, evaluated on the device: the lean small step's own cache look-up (re-use test, existence grid, candidate count, one-match shortcut,
 * count-limited search, inverse-distance blend, ComputeGaussian) on caller-given cache rows (npts <= 3000 x dim: pts, v1, v2; dim 6, 8, 10 or 12) and
 * one chain state per query (q, last_pss, ch_v1, ch_v2: nq x dim; queried, ss_score: nq).  grid_m 3 or 4; chosen_coords 0 = the grid over the leading
 * coordinates, 1 = over the ones the renderer would pick; device_grid 0 = the host's grid build, 1 = the device's.
 * out_int nq x 10 = [branch (0 isotropic, 1 re-use, 2 blend), matches, their rows in search order (5, -1 = none), cache-query and cache-hit counter
 * increments, hit of the generic kernel's query], out_w nq x 5 blend weights, out_chain nq x 3 x dim = chain v1, v2, last_pss afterwards,
 * out_gauss nq x (3 dim + 1) = mean, covL, invCov, logDet, out_generic nq x 2 x dim = v1, v2 of the generic kernel's query (zeros on a miss) */
int lmc_lean_query_probe(int dim, int npts, const float *pts, const float *v1, const float *v2, float mala_stepsize, float mala_stddev, int grid_m,
                         int chosen_coords, int device_grid, int nq, const float *q, const int *queried, const float *last_pss, const float *ch_v1,
                         const float *ch_v2, const float *ss_score, int *out_int, float *out_w, float *out_chain, float *out_gauss, float *out_generic);
/* Test probes of the bookkeeping launches the step kernels run on (device/kernels.hip, device/relocate.hip; host/list_probes.cpp): each copies the
 * caller's arrays to the device, calls the launch function the renderer calls, unchanged, on a stream, waits and copies the results back.  No context;
 * device 0.  All results are integers or copied words: the references (tests/list_cases.py) are exact.  Return 0, -1 on error.
 *   lmc_scan_probe              LaunchInclusiveScan: out[i] = in[0] + .. + in[i] (int32; n >= 1 -- the renderer's callers pass 256 or more, n = 0 is not a call)
 *   lmc_radix_sort_probe        LaunchRadixSort24 on n_max keys of 24 bits of which the first n count (n lives in device memory, 0 <= n <= n_max, n_max >= 1):
 *                               out_vals[p] = index of the p-th key in stable ascending order, out_keys[p] = that key; both n_max long, the entries from n on
 *                               hold the sentinel LMC_PROBE_SENTINEL
 *   lmc_sort_by_technique_probe LaunchSortByTechnique: the first n_list entries of list (chain ids < n_chains) grouped by next_kind[chain] >> 2 into out
 *                               (n_list entries; the rest of a max_entries-long device array is pre-filled with the sentinel and must stay: checked by the probe).
 *                               max_entries >= n_list: the capacity the (chunk, key) histogram is sized for (the renderer passes its chain count);
 *                               0 is legal with an empty list and launches nothing
 *   lmc_build_lists_probe       LaunchBuildLists over next_kind[N] (sort_plain 0 .. 3, lean_dims as the renderer passes it: bit 2 * (3 + path-length class) = that
 *                               cache is ready, bit 31 = lean launch without light sub-paths): out_large / out_generic / out_plain N entries each (sentinel beyond
 *                               the counts), out_counts[3], out_step_kind[N] with want_step_kind (else the launch gets no stepKind array and the pointer may be NULL)
 *   lmc_bins_compact_probe      LaunchBinsCompact: bin_of[N] (-1: takes no part), count[LMC_PROBE_BINS] = entries of the list per bin, list[n_list] ->
 *                               out_items[N] (sentinel beyond the total), out_start[LMC_PROBE_BINS]
 *   lmc_split_list_probe        LaunchSplitList: list[n_list] cut into `parts` (1 .. 4) sub-lists of `stride` entries each -> out_sub[parts * stride] (sentinel where
 *                               nothing is written), out_sub_count[parts]
 *   lmc_cache_push_probe        LaunchCachePush: push_dim[N] and push_data[N x 37] (per SLOT: pss[12], v1[12], v2[12], weight; the probe lays them out as the chains' pushData),
 *                               slot_of[N] chain -> slot or NULL (identity), initial_counts[4] rows already in the dims 6, 8, 10, 12.  Targets of LMC_PROBE_CACHE_ROWS
 *                               rows per dim, pre-filled with NaN of payload 0x7fc0beef; out_rows[4 x 3 x LMC_PROBE_CACHE_ROWS x 12] = pss | v1 | v2 of every dim
 *                               (row r, word k of array a of dim slot s at ((s * 3 + a) * ROWS + r) * 12 + k, the words from the dim on untouched),
 *                               out_weights[4 x ROWS], out_counts[4], out_push_dim[N] = push_dim afterwards
 *   lmc_reloc_plan_probe        LaunchRelocPlan (count, offsets, assign of LaunchRelocate): step_kind[N] (unsigned char), c[N], l[N] (words 0 and 1 of the
 *                               contribution), flags[N], placed_key[N]; count[1] = skipped_before going in.  out_count[2], out_members[N], out_sorted[N]
 *                               (sentinel beyond out_count[0] members ... beyond the members FOUND when the relocation is skipped: the lists are built either way) */
#define LMC_PROBE_SENTINEL (-0x5a5a5a5b)
#define LMC_PROBE_BINS 336
#define LMC_PROBE_CACHE_ROWS 3000
int lmc_scan_probe(int n, const int *in, int *out);
int lmc_radix_sort_probe(int n, int n_max, const unsigned *keys, int *out_vals, unsigned *out_keys);
int lmc_sort_by_technique_probe(int n_chains, const unsigned char *next_kind, int n_list, const int *list, int max_entries, int *out);
int lmc_build_lists_probe(int N, const unsigned char *next_kind, int sort_plain, unsigned lean_dims, int want_step_kind, int *out_large, int *out_generic,
                          int *out_plain, int *out_counts, unsigned char *out_step_kind);
int lmc_bins_compact_probe(int N, const int *bin_of, const int *count, int n_list, const int *list, int grid_blocks, int *out_items, int *out_start);
int lmc_split_list_probe(int n_list, const int *list, int parts, int stride, int grid_blocks, int *out_sub, int *out_sub_count);
int lmc_cache_push_probe(int N, const int *push_dim, const float *push_data, const int *slot_of, const int *initial_counts, float *out_rows, float *out_weights,
                         int *out_counts, int *out_push_dim);
int lmc_reloc_plan_probe(int N, const unsigned char *step_kind, const int *c, const int *l, const int *flags, const unsigned *placed_key, int without_gaussian_only,
                         int capacity, int skipped_before, int *out_count, int *out_members, int *out_sorted);
/* test probe, read-only: where the resident chains live once relocation is on (device/relocate.hip): slot_of[chain] and chain_id[slot], N ints each (either may
 * be NULL), copied after every stream of the context has drained.  Returns 0, -1 when relocation is off (or no chains are set up), -2 on error. */
int lmc_chain_slots(lmc_ctx *ctx, int *slot_of, int *chain_id);
/* ComputeGaussian (mala.cpp:7-52) + GaussianLogPdf (gaussian.cpp:24-36): out n x (3*dim+2) */
int lmc_gauss_probe(int n, int dim, const float *v1, const float *M, float ss, float shk, const float *sc, const float *offset, float *out);
/* Parity probes of the H2MC step's own launches (device/h2hess.hip, h2gauss.hip; reference: the evaluate_path_bidir_<c>_<l>_static_derv
 * programs with `hess`, h2mc.cpp:3-142, gaussian.cpp:24-36), item-major arrays:
 *   lmc_h2_hess_probe   n states of technique (c,l): primary n x (2L+1), vert n x V -> grad n x 16, hess n x 256 (row i at [i * dim], only
 *                       the triangle Eigen reads -- the UPPER triangle of the rows as delivered -- is written, the rest is 0), loglum n
 *   lmc_h2_gauss_probe  n gradients (n x 16) + Hessians (n x dim x dim, upper triangle read) -> the proposal Gaussian of each:
 *                       gauss n x 544 = [mean 16 | logDet | kind (0 dense, 1 isotropic early-out) | .. | covL at 32 (dim x dim) | invCov at 288],
 *                       and, with offset (n x dim) != NULL, px[n] = log N(-offset; mean, invCov^-1) */
int lmc_h2_hess_probe(int c, int l, int n, const float *primary, const float *scene38, const float *vert, float *loglum, float *grad, float *hess);
int lmc_h2_gauss_probe(int n, int dim, const float *grad, const float *hess, float sigma, const float *offset, float *gauss, float *px);
/* Test probes of the three wave-cooperative derivative launches ON A CALLER-GIVEN WORK LIST (device/gradcoop.hip k_mala_grad, h2hess.hip k_h2_hess,
 * h2gauss.hip k_h2_gauss; the list machinery of device/dh2coop.h; host/list_probes.cpp).  No context; device 0.  The two probes above are these with
 * everything in one bin, in identity order.  The work list is what the kernel reads: items[n_list] = chain ids grouped by bin, count[LMC_PROBE_BINS],
 * start[LMC_PROBE_BINS]: bin b = technique b / 8 x signature b % 8 lists items[start[b] .. start[b] + count[b]).  Refused on the host, before any device
 * call, through lmc_last_error (which names the argument): n_list < 1 or N < n_list (n = 0 is not a call), an item outside [0, N), an item listed
 * twice, a negative count, a bin that is not a range inside [0, n_list) or overlaps another (empty bins are not looked at), a listed chain whose (c, l)
 * -- whose dim, for the Gaussian -- is not that of the bin's technique, grid_blocks outside [1, 4096].  All counts zero is legal (the stage with no
 * takers): returns 0, writes nothing.  Every output is pre-filled with the float sentinel of bit pattern 0x7fc0beef, so the rows a launch wrote show.
 *   lmc_mala_grad_list_probe  N states: primary N x 17 (time, then 2 L samples), c[N], l[N], vert N x LMC_PROBE_VERT_WORDS (the technique's 238 + 59 (c + l - 3)
 *                             words, the rest unread), packed into the launch's records as lmc_h2_hess_probe packs them -> out N x 32 = the launch's rows:
 *                             [0, 16) gradient (dim words written) | [16] logLum
 *   lmc_h2_hess_list_probe    the same inputs -> out N x 288: [0, 16) gradient | [16] logLum | [32 ..) Hessian rows (stride dim; what the launch writes: the
 *                             upper triangle and the 2 x 2 diagonal blocks)
 *   lmc_h2_gauss_list_probe   N chains: dim[N] (even, 4 .. 16), grad N x 16, hess N x 256 (chain i's rows at stride dim[i]), flags[N] (only bit 64, F_GSEL,
 *                             is read), offset N x 16, stage 0 or 1, sigma -> gauss 2 x N x 544 (both buffers; a listed chain's record goes to buffer
 *                             (F_GSEL set) != (stage != 0), layout as lmc_h2_gauss_probe's), px[N] (written at stage 1 only)
 *   lmc_coop_plan_probe       no device: for kernel 0 (k_mala_grad), 1 (k_h2_hess), 2 (k_h2_gauss) and technique index tech (0 .. 41: (c + l - 1)(c + l) / 2 - 3 + l)
 *                             the states one task takes and the words of a state's record a wave stages (k_h2_gauss: the words of a Hessian record) */
#define LMC_PROBE_VERT_WORDS 592
int lmc_mala_grad_list_probe(int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38, int n_list, const int *items,
                             const int *count, const int *start, int grid_blocks, float *out);
int lmc_h2_hess_list_probe(int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38, int n_list, const int *items,
                           const int *count, const int *start, int grid_blocks, float *out);
int lmc_h2_gauss_list_probe(int N, const int *dim, const float *grad, const float *hess, const int *flags, const float *offset, int stage, float sigma, int n_list,
                            const int *items, const int *count, const int *start, int grid_blocks, float *gauss, float *px);
int lmc_coop_plan_probe(int kernel, int tech, int *states_per_task, int *rec_words);
/* Test probe of the shading functions (device/dshade.h through device/shade_probe.hip; host/shade_probes.cpp).  No context; device 0.  One case per lane
 * in 64-thread blocks; op 0 = EvalTex on one of a material's four texture references at st, 1 = BsdfEvaluate<G>, 2 = BsdfSample<G>, with G = (glossy != 0)
 * the template argument the kernels are instantiated for (G = 0 runs the Lambertian functions on any record).
 *   materials     n_mat rows of LMC_SHADE_MAT_WORDS 32-bit words in the device's record layout (device/dscene.h DMaterial):
 *                 [type (int 0 Lambertian, 1 Phong, 2 rough dielectric) | twoSided (int) | Kd | Ks | Kt | expOrAlpha | eta | invEta | KsWeight], a texture
 *                 reference = [bitmap (int: index into the bitmap list, -1 = constant) | value[3] | sScale | tScale].  The rows go through the packing a
 *                 scene's materials go through (texel pool, inline texture headers).
 *   bitmaps       bitmap_wh n_bitmaps x [W, H], bitmap_gamma[n_bitmaps], texels = the bitmaps' 3 W H floats each, back to back (n_texels floats in all)
 *   case_ints     n x LMC_SHADE_INT_WORDS: [material index | adjoint | texture slot (0 Kd, 1 Ks, 2 Kt, 3 expOrAlpha; op 0 only)]
 *   case_in       n x LMC_SHADE_IN_WORDS:  [wi 0..2 | normal 3..5 | wo 6..8 | st 9..10 | rnd 11..12 | uDiscrete 13 | and the values the in / out arguments
 *                 hold going in: pdf 14 | revPdf 15 | cosWo 16 | contrib 17..19] (wo is an input of op 1 and the value going in of op 2)
 *   out           n_rows x LMC_SHADE_OUT_WORDS: [wo 0..2 | contrib 3..5 | cosWo 6 | pdf 7 | revPdf 8] as the call left them -- a word the function did not
 *                 write holds the bits that went in; op 0 writes the texture's value to contrib
 *   out_ok        n_rows: BsdfSample's return value (0 / 1); 1 for op 0 and 1
 * n_rows >= n is the length of the two outputs: both are pre-filled on the device with LMC_PROBE_SENTINEL (out_ok) and the float of bit pattern
 * LMC_SHADE_UNTOUCHED_BITS (out), and the rows from n on must come back so.  No input may be NaN or infinite (the look-up converts st to integers).
 * Refused on the host, before any device call, through lmc_last_error (which names the argument): an unknown op, n_mat < 1, n < 1, n_rows < n, a null
 * pointer, a type outside 0 .. 2, a bitmap index outside [-1, n_bitmaps), a case's material index outside [0, n_mat) or (op 0) texture slot outside
 * 0 .. 3, W or H below 1, n_texels shorter than the sum of 3 W H. */
#define LMC_SHADE_MAT_WORDS 29
#define LMC_SHADE_INT_WORDS 3
#define LMC_SHADE_IN_WORDS 20
#define LMC_SHADE_OUT_WORDS 9
#define LMC_SHADE_UNTOUCHED_BITS 0x7fc0beefu
int lmc_shade_probe(int op, int glossy, int n_mat, const float *materials, int n_bitmaps, const int *bitmap_wh, const float *bitmap_gamma, const float *texels,
                    long long n_texels, int n, int n_rows, const int *case_ints, const float *case_in, int *out_ok, float *out);
/* HBM counter calibration: `reps` launches of a kernel that reads n_words floats and writes n_words floats with the
 * chain state's access pattern (4 B per lane, SoA, unit stride).  Run under rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
 * to obtain the bytes-per-count factors profiles/pmc_step_kernel.json applies.  Returns 0 on success. */
int lmc_stream_probe(long long n_words, int reps);

/* Checkpoint and resume (INTEGRATION.md "Checkpoint and resume"; device/checkpoint.hip).  A checkpoint is one file: a header with the fingerprint of
 * everything the chain states depend on (a content hash of the scene's files, force_diffuse, film size, depths, seed offset, use_gradient,
 * max-derivatives-depth and the <dpt> options the chain loop reads), the job's shape, the steps and wall seconds so far; the job-wide state (init
 * results, gradient caches, counters, film); and one record per chain of the job in chain order -- independent of the slots the chains lived in, of
 * the schedule that ran them and of the number of in-process members that held them.
 * save: legal between two lmc_chains_step calls, after lmc_chains_init or a load; drains the context's streams, writes path + ".tmp" and renames
 *       it, and changes nothing in the context.  Refused before init, on a film that already holds a reduced sum, and inside an RCCL job.
 * load: takes the place of lmc_chains_init on a context created from the same scene and overrides with the same options set; the fingerprint is
 *       compared field by field and a mismatch (or a wrong magic / version, or a truncated file) returns -1 with the field's name in
 *       lmc_last_error, leaving the context as it was.  resident_steps / resident_lanes / resort_every / resort_first / overlap / timing and
 *       LMC_RELOCATE are the loading context's own.  The chains come back in the identity layout, as after init.
 * group calls: the same file format; a file written by one context or by a group of any size loads into one context or into a group of any size
 *       (chains split like lmc_group_chains_init); every member receives the job-wide state, member 0 alone the film, counters and weight sum.
 * info: host only; the header as a JSON document (lmc_scene_dump's convention: at most cap - 1 characters + NUL, returns the full length, -1 on error). */
int lmc_checkpoint_save(lmc_ctx *ctx, const char *path);
int lmc_checkpoint_load(lmc_ctx *ctx, const char *path);
int lmc_group_checkpoint_save(lmc_ctx **ctxs, int n, const char *path);
int lmc_group_checkpoint_load(lmc_ctx **ctxs, int n, const char *path);
long long lmc_checkpoint_info(const char *path, char *json, long long cap);

/* Exact film (INTEGRATION.md "Exact film"): lmc_set_option "film_exact" = 1 (default 0; 1 when the environment has LMC_FILM_EXACT=1) makes the MLT
 * film a W*H*3 array of signed 64-bit fixed-point words added with integer atomics, so the film is a pure function of the chains' trajectories: bit-equal
 * from run to run, across slot layouts and schedules, across members and ranks, and across a checkpoint.
 *   conversion  q = llrint((double)v * 4294967296.0): one unit is 2^-32 of the float film's unit; the product is exact in double, one round to nearest even
 *   range       a splat with a component |v| >= 2^30 is dropped WHOLE and counted in film_overflow (a stated deviation from the float film)
 * Set the option BEFORE the context's first lmc_chains_init / lmc_checkpoint_load: once a context has chains it keeps its mode for life (a later
 * lmc_chains_init does not change it).  It takes effect at that first lmc_chains_init / lmc_checkpoint_load; changing it on a context whose chains are set up is refused (-1, the context
 * stays usable).  All members of an in-process group must have the same mode.  In exact mode
 *   lmc_film_read         converts on the device, float(double(q) * 2^-32), and returns W*H*3 floats, un-normalised, as in float mode
 *   lmc_film_read_fixed   the raw words (W*H*3); -1 in float mode
 *   lmc_film_overflow     *n = splats dropped by the range rule since the film was last cleared (always 0 in float mode); per context, and after
 *                         lmc_film_allreduce the sum over the ranks
 *   lmc_film_clear        zeroes the words and the counter
 *   lmc_film_device_ptr   returns the int64 buffer and its word count: the ELEMENT TYPE FOLLOWS THE MODE (float in float mode)
 *   lmc_group_film_reduce / lmc_film_allreduce   sum the int64 words (ncclInt64): exact in any order.  ALL RANKS of a communicator must have the same
 *                         mode: lmc_film_allreduce takes the element type and count from the local mode and does not compare them across ranks
 *                         (the in-process group is checked; rank processes are the caller's to configure alike)
 *   checkpoints           store the int64 film (format version 2, "film_format":"fixed64" in lmc_checkpoint_info); float-mode files are version 1,
 *                         byte for byte as before; a file loads only into a context of its own mode
 * The direct-lighting and mc-integrator films (lmc_direct_read, lmc_mc_read) are float in either mode; the mc film has an exact mode of its own,
 * "mc_film_exact" (above). */
int lmc_film_read_fixed(lmc_ctx *ctx, long long *out);
int lmc_film_overflow(lmc_ctx *ctx, long long *n);
/* test probe: n splats (screen_xy n x 2 in [0,1)^2, rgb n x 3) through the device's splat routine into a fresh W x H film, one launch of n lanes in
 * 64-thread blocks.  exact != 0: out_fixed = the W*H*3 words, *overflow = dropped splats, out_float = the converted film; exact == 0: out_float = the
 * float film (out_fixed must be NULL).  Any output may be NULL. */
int lmc_film_splat_probe(int W, int H, int n, const float *screen_xy, const float *rgb, int exact, long long *out_fixed, float *out_float, long long *overflow);

/* ---- Chain diagnostics (device/chaindiag.hip, host/chaindiag.cpp; INTEGRATION.md "Chain diagnostics").  Opt-in; a context that uses none of it runs
 * exactly the launches it ran before.
 *
 * Rows.  lmc_chain_rows gathers the rows of n chosen chains ON THE DEVICE (one wave per chain; lmc_chain_summary downloads every path buffer of
 * every chain) and copies n * LMC_ROW_WORDS floats out.  chain_ids are GLOBAL chain ids inside this context's [chain_begin, chain_end), in any
 * order, repeats allowed; any other id is refused (-1, a message, nothing written).  which = 0 current, 1 init states.  A row:
 *   words  0..15  the 16 header words of lmc_chain_summary, bit for bit (and with the summary's meaning for an INVALID state: same arrays, same words)
 *   words 16..39  pss[0..23] in GetPathPss order; the first 16 are the summary's words 16..31
 *   word  40      the launch that ran the step which produced the state: 1 large, 2 generic small, 3 lean small, 0 the chain did not step (its
 *                 samples are used up), -1 outside a trace
 *   word  41      adjacentReject: 0 exactly when the chain's last step accepted its proposal
 *   word  42      the chain's flags word (device/dchain.h F_*), as a float
 *   words 43..47  0
 * For which == 1 the words 40..42 are 0.
 *
 * Traces.  Between lmc_chain_trace_begin and _end every lock step ends by queueing the row gather of the n tracked chains on the step stream, into a
 * device buffer of capacity_steps x n x LMC_ROW_WORDS floats: no host wait, no copy.  The row of step s is what lmc_chain_rows would return after
 * step s, word 40 filled.  When the buffer is full further steps are not recorded but counted.  lmc_chain_trace_read waits for the step stream,
 * copies out rows[n_steps][n][LMC_ROW_WORDS] (cap_steps, the steps `rows` has room for, must be at least the steps buffered: a smaller one is refused;
 * rows == NULL only reports *first_step, *n_steps and *dropped and changes nothing), reports the step index of the first row
 * (steps are counted from 1 after lmc_chains_init; after a checkpoint load from the loaded count), then empties the buffer and zeroes the drop
 * count; recording goes on.  Every context -- a member of a group, a rank of a job -- traces its own chains.  lmc_chains_init and
 * lmc_checkpoint_load close an open trace.
 * While a trace is open or the step table is on, the resident schedule ("resident_steps") is not taken: a resident launch cannot be observed between
 * its mutations, and by that schedule's contract the trajectories are the same in lock step; lmc_resident_stats shows the lock steps run.
 * Refused (-1, a message, the context unchanged and usable): begin before lmc_chains_init or while a trace is open, n <= 0, capacity_steps <= 0, an
 * id outside the context's range, a buffer that cannot be allocated (the message names the bytes); read / end without an open trace.
 *
 * Step table.  lmc_set_option "step_table" = 1 counts from the next lock step on, 0 stops counting (the table keeps its figures).  lmc_step_table copies
 * out[3][13][13][2]: out[kind - 1][c][l][0] = chain-steps of that launch kind (1 large, 2 generic small, 3 lean small) whose chain's CURRENT state
 * after the step has technique (c, l) = (camDepth, lightDepth); [1] = those of them whose proposal was accepted.  clear != 0 zeroes the table behind
 * the copy.  Integer counts, exact and independent of slot order. */
#define LMC_ROW_WORDS 48
int lmc_chain_rows(lmc_ctx *ctx, int which, const int *chain_ids, int n, float *out);
int lmc_chain_trace_begin(lmc_ctx *ctx, const int *chain_ids, int n, int capacity_steps);
int lmc_chain_trace_read(lmc_ctx *ctx, float *rows, int cap_steps, long long *first_step, int *n_steps, long long *dropped);
int lmc_chain_trace_end(lmc_ctx *ctx);
int lmc_step_table(lmc_ctx *ctx, long long *out, int clear);
/* Pending splat lists.  lmc_chain_splats gathers, on the device, the pending splat list of n chosen chains -- the contributions a rejected (or partly
 * accepted) step splats again, the list row word 15 only counts.  chain_ids follow the rules of lmc_chain_rows.  counts[k] = the length of chain k's list;
 * out[(k * cap + e) * LMC_SPLAT_WORDS ..] = x, y (screen position in [0,1)^2), r, g, b (the values as stored: scaled, not yet weighted by the acceptance)
 * and the entry's label c * 16 + l as a float, -1 when "film_layers" is off; e < min(counts[k], cap), the entries behind are zero.  cap = 1 ..
 * LMC_SPLAT_MAX_ENTRIES.  Of an INVALID state the list means nothing (the chain loop does not splat it). */
#define LMC_SPLAT_WORDS 6
#define LMC_SPLAT_MAX_ENTRIES 85
int lmc_chain_splats(lmc_ctx *ctx, const int *chain_ids, int n, int cap, float *out, int *counts);

/* ---- Layered MLT film (INTEGRATION.md "Layered MLT film"; device/dchain.h ChainFilmLayers, device/step_*_layers.hip, host/filmlayers.cpp).
 * lmc_set_option "film_layers" = 1 (by path length) or 2 (by technique), default 0 (off: the films and the kernels above).  The option follows the rules of
 * "film_exact": set BEFORE the context's first lmc_chains_init, kept for life, a change on a context whose chains are set up is refused (-1, the context
 * stays usable).  Exact mode only: with "film_layers" set and "film_exact" = 0 lmc_chains_init returns -1 with a message naming both options.
 *   the film     n_layers exact films of W*H*3 int64 words one after the other and ONE overflow word.  Every splat of the chain loop goes to the layer of
 *                its contribution's technique (c, l) = (camDepth, lightDepth); pixel, finite and range rules per contribution are those of the exact
 *                film, so the layers sum to the unlayered exact film WORD FOR WORD, with the same chain states and counters.
 *   numbering    that of "mc_layers" (above): D = maxdepth (1 .. 12); 1: D layers, layer L - 1; 2: D (D + 3) / 2 layers, layer (L - 1)(L + 2) / 2 + l.
 *                A technique outside the table is dropped whole and counted in the overflow word, never written.
 *   labels       the techniques of the pending splat lists live in one byte c * 16 + l per entry, indexed by chain id (lmc_chain_splats reads them)
 *   the total    lmc_film_read, lmc_film_read_fixed, lmc_film_overflow and lmc_film_device_ptr apply to the sum of the layers (int64 adds), made when
 *                they are called: a caller that ignores the layers sees the unlayered exact film, the same words
 *   lmc_film_layer_info        *mode, *n_layers of the film the context holds (n_layers = 0: unlayered); cl receives at most cap pairs, (L, -1) in length
 *                              mode, (c, l) in technique mode
 *   lmc_film_read_layer        one layer as W*H*3 floats, converted like lmc_film_read and un-normalised
 *   lmc_film_read_layer_fixed  one layer's raw words
 *   lmc_film_clear             zeroes every layer and the counter
 *   lmc_group_film_reduce      sums the members' films layer by layer (and the overflow words); all members must have the same mode: a mixed group is
 *                              refused by lmc_group_chains_init and lmc_group_film_reduce, as a mixed "film_exact" is
 * While the mode is on the resident schedule ("resident_steps") is not taken, exactly as while a trace is open: by that schedule's contract the
 * trajectories are the same in lock step; lmc_resident_stats shows the lock steps run.
 * Refused in this version (-1, a message naming film_layers, nothing written, the context usable): H2MC contexts (at lmc_chains_init), lmc_checkpoint_save /
 * _load and their group forms, lmc_film_allreduce on a communicator of more than one rank, a layer index outside [0, n_layers), the layer readers on an
 * unlayered context.
 * lmc_film_layer_splat_probe (test probe): n splats (screen_xy n x 2, rgb n x 3, techniques cl n x 2 = camDepth, lightDepth) through the device's layered
 * splat routine into a fresh W x H film of mode / D.  out_fixed: n_layers * W*H*3 words; *overflow: the film's overflow word (range rule AND outside the
 * table); *outside: the finite splats whose technique is outside the table.  Any output may be NULL. */
int lmc_film_layer_info(lmc_ctx *ctx, int *mode, int *n_layers, int *cl, int cap);
int lmc_film_read_layer(lmc_ctx *ctx, int layer, float *rgb);
int lmc_film_read_layer_fixed(lmc_ctx *ctx, int layer, long long *words);
int lmc_film_layer_splat_probe(int W, int H, int mode, int D, int n, const float *screen_xy, const float *rgb, const int *cl, long long *out_fixed, long long *overflow,
                               long long *outside);

#ifdef __cplusplus
}
#endif
#endif
