// dpt_amd: the reference's process surface (`dpt [--seedoffset N] scene.xml ...`, main.cpp:30-118 of the reference) on top of the C
// ABI of liblmc_hip.so.  Same scene XML, same <dpt> keys, same output naming (<film filename>_timeuse_<seconds>s.exr written next to the
// scene, mlt.cpp:208) and the same stdout lines ("Average brightness:", "Elapsed time:", "Done!").  The scene's <string integrator> is
// dispatched on first, as main.cpp:92-104 does:
//   mc    PathTrace (pathtrace.cpp:14-78) through lmc_mc_render: spp samples per pixel, bidirectional or not as <dpt> says, "Elapsed time:"
//         around the render.  The one deliberate deviation: the reference computes this film and writes nothing (pathtrace.cpp:77,
//         main.cpp:95); dpt_amd writes it like the MLT branch does.  --seedoffset feeds the streams' seed offset (the reference's PathTrace
//         ignores it; with the default 0 the two agree).  --gpus / --devices split the stream range into contiguous shards, one context
//         per device, and the films are summed on member 0's device (lmc_group_mc_render).  The MLT-only flags (--chains, --resident, --init-threads) are ignored.
//   mcmc  the LMC path: mala = true or h2mc = true; plain MLT (both false) is refused.
// Extra flags (not in the reference): --chains N (Markov chains resident on the GPUs, default: <dpt numchains>), --init-threads V (MLTInit
// streams, default 65536), --device D, --force-diffuse, --maxdepth D, --resident K (the resident schedule, lmc_set_option "resident_steps": up to K mutations of every chain per launch once the gradient caches are frozen; H2MC
// renders stay in lock step), and
// --gpus N (devices 0 .. N-1) / --devices a,b,.. (an explicit list; a device may appear more than once: bring-up on one GPU): the chains are
// sharded over the listed devices as ranks of ONE job (lmc_group_*: MLTInit sharded by init stream, contiguous chain-id ranges, the gradient
// cache's pushes exchanged while it fills -- the trajectories of a single device holding all the chains), and the per-device films are summed
// on the devices before the image is written (mlt.cpp:203-207 merges its per-thread films the same way).
// Checkpoints (lmc_checkpoint_* / lmc_group_checkpoint_*, INTEGRATION.md "Checkpoint and resume"): --checkpoint FILE writes the render's state at the
// end of the run, with --checkpoint-every S also every S steps; --max-steps S stops this invocation after S steps, writes the checkpoint and the
// image of what has been rendered so far; --resume FILE skips MLTInit and continues to the scene's spp (the direct pre-pass is recomputed: it is
// deterministic).  The _timeuse_<seconds>s suffix carries the seconds of all legs.  All of it works with --gpus / --devices.
// --exact-film (lmc_set_option "film_exact", INTEGRATION.md "Exact film"): the MLT film is accumulated in 64-bit fixed point, so the written image does
// not depend on the order of the splats -- the same bytes from run to run, for any --gpus / --devices, with or without --resident, and across
// --checkpoint / --resume.  A resume takes the mode from the file; --exact-film on a float-film checkpoint is an error.  The EXR is produced from the
// converted float film exactly as in float mode.
// On an mc scene --exact-film selects the exact mc film (lmc_set_option "mc_film_exact", INTEGRATION.md "Exact mc film"): the same words for any --gpus /
// --devices list, for any cut into legs, and from run to run.  There --spp N overrides <dpt spp>, --max-spp K renders the sample indices below K only
// and writes the image with divisor K, --checkpoint F writes the film's state file (lmc_mc_save) at the end and --resume F loads one and renders what
// its coverage lacks of [0, nTiles * spp); both need the exact film (a resume takes the mode from the file).
// --mc-layers length|technique (mc scenes only; lmc_set_option "mc_layers", INTEGRATION.md "Layered mc film"): the render split by path length or by technique.
// The usual EXR holds the sum of the layers; beside it every non-empty layer is written under the same name with _L<length> (two digits) or
// _c<camDepth>_l<lightDepth> before .exr.  One device, no --checkpoint / --resume in this version.
// --film-layers length|technique (mcmc scenes; lmc_set_option "film_layers", INTEGRATION.md "Layered MLT film"): the MLT film split the same way.  It implies
// --exact-film; the usual EXR is, byte for byte, the one an --exact-film run without the flag writes, and every non-empty layer is written beside it with
// the suffixes above, scaled as the indirect film is before the direct film is added (1 / spp).  Works with --gpus / --devices; with --checkpoint /
// --resume it is an error at start.
// Chain diagnostics (mcmc scenes on one device; include/lmc_abi.h "Chain diagnostics"): --trace-chains a,b,.. --trace-file F [--trace-steps S, default 1024]
// records the rows of the listed chains over the first S steps of this invocation and writes F (little-endian: "LMCTRACE", u32 version 1, u32 row words,
// u32 n, u32 steps, i64 first step, n x i32 chain ids, then steps x n x row-words floats); --step-table prints the non-empty cells of lmc_step_table,
// one line each ("kind c l steps accepted"), before "Done!".  Either keeps the render in lock step (--resident then has no effect).
// --help lists the flags.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "lmc_abi.h"

// a number of a flat JSON document (lmc_checkpoint_info)
static double JsonNumber(const std::string &json, const char *key) {
    const std::string k = std::string("\"") + key + "\":";
    const size_t at = json.find(k);
    return at == std::string::npos ? 0.0 : atof(json.c_str() + at + k.size());
}

static double Opt(lmc_ctx *ctx, const char *name) {
    double v = 0;
    if (lmc_get_option(ctx, name, &v) != 0) {
        fprintf(stderr, "%s\n", lmc_last_error());
        exit(1);
    }
    return v;
}

// the mc branch's flags
struct McFlags {
    bool exactFilm = false;
    int spp = 0, maxSpp = 0;  // --spp / --max-spp (0: not given)
    std::string checkpointPath, resumePath;
    int layers = 0;  // --mc-layers: 1 length, 2 technique
};

// integrator = mc: the stream range [0, nTiles * spp) split into contiguous shards, one per context, rendered concurrently and summed on member 0's
// device (lmc_group_mc_render).  With --max-spp K only the sample indices below K are rendered and the image is written with divisor K; --resume
// renders what the file's coverage lacks of that range.
static int RenderMC(const std::string &filename, std::vector<lmc_ctx *> &ctxs, const McFlags &F) {
    lmc_ctx *ctx = ctxs[0];
    int info[8];
    lmc_info(ctx, info);
    const int W = info[0], H = info[1], sceneSpp = F.spp > 0 ? F.spp : (int)Opt(ctx, "spp"), nDev = (int)ctxs.size();
    const int spp = F.maxSpp > 0 ? std::min(F.maxSpp, sceneSpp) : sceneSpp;  // what this invocation's film ends with, and its divisor
    const long long nTiles = (long long)((W + 15) / 16) * ((H + 15) / 16), total = nTiles * spp;
    bool exact = F.exactFilm || Opt(ctx, "mc_film_exact") != 0;
    if (!F.resumePath.empty()) {  // a resume takes the mode from the file: a state file holds an exact film
        char json[4096];
        if (lmc_mc_file_info(F.resumePath.c_str(), json, sizeof(json)) < 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        exact = true;
    }
    if (!exact && (!F.checkpointPath.empty() || !F.resumePath.empty())) {
        fprintf(stderr, "--checkpoint / --resume on an integrator=mc scene need the exact film: add --exact-film\n");
        return 2;
    }
    for (lmc_ctx *c : ctxs)
        if (lmc_set_option(c, "mc_film_exact", exact ? 1 : 0) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
    if (F.layers != 0) {
        if (nDev > 1 || !F.checkpointPath.empty() || !F.resumePath.empty()) {
            fprintf(stderr, "--mc-layers: a layered mc film is rendered on one device and has no state file in this version (no --gpus / --devices list, --checkpoint or --resume)\n");
            return 2;
        }
        if (lmc_set_option(ctx, "mc_layers", F.layers) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
    }
    if (exact) printf("Exact film: 64-bit fixed-point accumulation\n");
    if (nDev > 1) printf("%lld sample streams sharded over %d devices\n", total, nDev);
    auto t0 = std::chrono::steady_clock::now();
    if (F.layers != 0) {
        if (lmc_mc_render(ctx, spp, 0, total) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
    } else if (F.resumePath.empty()) {
        if (lmc_group_mc_render(ctxs.data(), nDev, spp, 0, total) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
    } else {
        if (lmc_mc_load(ctx, F.resumePath.c_str()) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        std::vector<long long> held(2 * 4096);
        const int nHeld = lmc_mc_coverage(ctx, held.data(), 4096);
        if (nHeld < 0 || nHeld > 4096) {
            fprintf(stderr, "%s\n", nHeld < 0 ? lmc_last_error() : "--resume: the file's coverage has more than 4096 ranges");
            return 1;
        }
        if (nHeld > 0 && held[2 * nHeld - 1] > total) {
            fprintf(stderr, "--resume: %s holds stream ids beyond the %lld of %d spp\n", F.resumePath.c_str(), total, spp);
            return 2;
        }
        long long at = 0, rendered = 0;
        for (int k = 0; k <= nHeld && at < total; k++) {  // the gaps of the coverage within [0, total)
            const long long gapEnd = k < nHeld ? std::min(held[2 * k], total) : total;
            if (gapEnd > at) {
                if (lmc_group_mc_accumulate(ctxs.data(), nDev, spp, at, gapEnd) != 0) {
                    fprintf(stderr, "%s\n", lmc_last_error());
                    return 1;
                }
                rendered += gapEnd - at;
            }
            if (k < nHeld) at = std::max(at, held[2 * k + 1]);
        }
        if (rendered == 0 && lmc_mc_accumulate(ctx, spp, 0, 0) != 0) {  // nothing was missing: the divisor is still this invocation's
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        printf("Resumed from %s: %lld of %lld sample streams were missing\n", F.resumePath.c_str(), rendered, total);
    }
    const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Elapsed time:%g\n", elapsed);  // pathtrace.cpp:74-75
    std::vector<float> img((size_t)W * H * 3, 0.0f);
    long long st[2] = {0, 0}, dropped = 0;
    if (lmc_mc_read(ctx, img.data()) != 0 || lmc_mc_stats(ctx, st) != 0 || lmc_mc_overflow(ctx, &dropped) != 0) {
        fprintf(stderr, "%s\n", lmc_last_error());
        return 1;
    }
    if (!F.checkpointPath.empty()) {
        if (lmc_mc_save(ctx, F.checkpointPath.c_str()) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        printf("Checkpoint written to %s (%d spp)\n", F.checkpointPath.c_str(), spp);
    }
    std::string dir = filename.rfind('/') != std::string::npos ? filename.substr(0, filename.rfind('/') + 1) : "";
    std::string out = dir + lmc_output_name(ctx) + "_timeuse_" + std::to_string(elapsed) + "s.exr";
    if (lmc_image_write_exr(out.c_str(), img.data(), W, H) != 0) {
        fprintf(stderr, "%s\n", lmc_last_error());
        return 1;
    }
    if (F.layers != 0) {  // every non-empty layer beside the image
        int mode = 0, nLayers = 0, written = 0;
        std::vector<int> cl(2 * 128);
        if (lmc_mc_layer_info(ctx, &mode, &nLayers, cl.data(), 128) != 0 || nLayers > 128) {
            fprintf(stderr, "%s\n", nLayers > 128 ? "--mc-layers: more than 128 layers" : lmc_last_error());
            return 1;
        }
        std::vector<float> layer((size_t)W * H * 3);
        for (int k = 0; k < nLayers; k++) {
            if (lmc_mc_read_layer(ctx, k, layer.data()) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            if (std::all_of(layer.begin(), layer.end(), [](float v) { return v == 0.0f; })) continue;
            char tag[64];
            if (mode == 1) snprintf(tag, sizeof(tag), "_L%02d", cl[2 * k]);
            else
                snprintf(tag, sizeof(tag), "_c%d_l%d", cl[2 * k], cl[2 * k + 1]);
            const std::string name = out.substr(0, out.size() - 4) + tag + ".exr";
            if (lmc_image_write_exr(name.c_str(), layer.data(), W, H) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            written++;
        }
        printf("Layered film (%s): %d of %d layers are non-empty and written beside the image\n", mode == 1 ? "by path length" : "by technique", written, nLayers);
    }
    if (dropped > 0) printf("Exact film: %lld contributions with a component of 2^30 or more were dropped\n", dropped);
    printf("%lld paths, %lld contributions, %.1f M paths/s, wrote %s\n", st[0], st[1], st[0] / elapsed * 1e-6, out.c_str());
    return 0;
}

static std::vector<int> IntList(const std::string &list) {
    std::vector<int> v;
    for (size_t b = 0; b <= list.size();) {
        const size_t e = list.find(',', b) == std::string::npos ? list.size() : list.find(',', b);
        if (e > b) v.push_back(std::stoi(list.substr(b, e - b)));
        b = e + 1;
    }
    return v;
}

// the open trace of `ctx` read and written as a trace file (layout: head of this file)
static int WriteTrace(lmc_ctx *ctx, const std::vector<int> &ids, int capSteps, const std::string &path) {
    const size_t n = ids.size();
    std::vector<float> rows((size_t)capSteps * n * LMC_ROW_WORDS);
    long long first = 0, dropped = 0;
    int steps = 0;
    if (lmc_chain_trace_read(ctx, rows.data(), capSteps, &first, &steps, &dropped) != 0 || lmc_chain_trace_end(ctx) != 0) {
        fprintf(stderr, "--trace-file: %s\n", lmc_last_error());
        return 1;
    }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "--trace-file: cannot write %s\n", path.c_str());
        return 1;
    }
    const unsigned head[4] = {1u, (unsigned)LMC_ROW_WORDS, (unsigned)n, (unsigned)steps};
    bool ok = fwrite("LMCTRACE", 1, 8, f) == 8 && fwrite(head, 4, 4, f) == 4 && fwrite(&first, 8, 1, f) == 1 && fwrite(ids.data(), 4, n, f) == n;
    const size_t words = (size_t)steps * n * LMC_ROW_WORDS;
    ok = ok && fwrite(rows.data(), 4, words, f) == words;
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        fprintf(stderr, "--trace-file: cannot write %s\n", path.c_str());
        return 1;
    }
    printf("Chain trace: %zu chains, steps %lld .. %lld (%lld later steps not recorded), wrote %s\n", n, first, first + steps - 1, dropped, path.c_str());
    return 0;
}

static void PrintHelp() {
    printf("usage: dpt_amd [flags] scene.xml ...\n"
           "  --seedoffset N              seed offset of the render's random streams\n"
           "  --max-derivatives-depth D   techniques longer than D get isotropic proposals (default 8)\n"
           "  --chains N                  Markov chains resident on the GPUs (default: <dpt numchains>)\n"
           "  --init-threads V            MLTInit streams (default 65536)\n"
           "  --device D                  HIP device ordinal\n"
           "  --gpus N | --devices a,b,.. shard the render over several devices\n"
           "  --force-diffuse             every material Lambertian\n"
           "  --maxdepth D                override <dpt maxdepth>\n"
           "  --resident K                resident schedule: up to K mutations per launch once the caches are frozen\n"
           "  --checkpoint FILE [--checkpoint-every S] [--max-steps S] | --resume FILE\n"
           "  --exact-film                64-bit fixed-point film, bit-equal from run to run\n"
           "  --spp N, --max-spp K        integrator=mc: samples per pixel / render the sample indices below K only\n"
           "  --mc-layers length|technique   integrator=mc: the film split by path length or by technique\n"
           "  --film-layers length|technique integrator=mcmc: the MLT film split the same way (implies --exact-film; no --checkpoint / --resume)\n"
           "  --trace-chains a,b,..       integrator=mcmc, one device: record the rows of these chains after every step ...\n"
           "  --trace-file FILE           ... and write them to FILE (\"LMCTRACE\", version 1; langevin-mcmc_amd trace_file_read)\n"
           "  --trace-steps S             ... over the first S steps of this invocation (default 1024)\n"
           "  --step-table                integrator=mcmc, one device: print chain-steps and accepted steps per launch kind and technique\n"
           "  --help                      this text\n");
}

int main(int argc, char *argv[]) {
    if (argc <= 1) return 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) {
            PrintHelp();
            return 0;
        }
    printf("Langevin MCMC dpt (MI355X back end)\n");
    int seedoffset = 0, device = 0, forceDiffuse = 0, maxDepth = 0, initThreads = 65536, maxDervDepth = 8, resident = 0;
    long long chains = 0, maxSteps = -1, checkpointEvery = 0;
    std::string checkpointPath, resumePath;
    bool exactFilm = false;
    int mcSpp = 0, mcMaxSpp = 0;  // --spp / --max-spp (integrator = mc)
    int mcLayers = 0;              // --mc-layers length|technique (integrator = mc)
    int filmLayers = 0;            // --film-layers length|technique (integrator = mcmc)
    std::vector<int> traceChains;  // --trace-chains / --trace-file / --trace-steps, --step-table (integrator = mcmc, one device)
    std::string traceFile;
    int traceSteps = 1024;
    bool traceChainsGiven = false, traceStepsGiven = false, stepTable = false;
    bool mltFlags = false;  // --chains / --resident / --init-threads given (ignored by integrator = mc)
    std::vector<int> devices;
    std::vector<std::string> filenames;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--seedoffset") seedoffset = std::stoi(argv[++i]);
        else if (a == "--max-derivatives-depth") maxDervDepth = std::stoi(argv[++i]);  // main.cpp:59-60: techniques longer than this get isotropic proposals
        else if (a == "--compile-pathlib" || a == "--compile-bidirpathlib" || a == "--compile-bidirpathlib2") {
            printf("%s: nothing to compile, the path programs are part of liblmc_hip.so\n", a.c_str());
        } else if (a == "--chains") chains = std::stoll(argv[++i]), mltFlags = true;
        else if (a == "--init-threads") initThreads = std::stoi(argv[++i]), mltFlags = true;
        else if (a == "--device") device = std::stoi(argv[++i]);
        else if (a == "--gpus") {
            const int n = std::stoi(argv[++i]);
            devices.clear();
            for (int d = 0; d < n; d++) devices.push_back(d);
        } else if (a == "--devices") {
            devices.clear();
            std::string list = argv[++i];
            for (size_t b = 0; b <= list.size();) {
                const size_t e = list.find(',', b) == std::string::npos ? list.size() : list.find(',', b);
                if (e > b) devices.push_back(std::stoi(list.substr(b, e - b)));
                b = e + 1;
            }
        } else if (a == "--force-diffuse") forceDiffuse = 1;
        else if (a == "--maxdepth") maxDepth = std::stoi(argv[++i]);
        else if (a == "--resident") resident = std::stoi(argv[++i]), mltFlags = true;
        else if (a == "--checkpoint") checkpointPath = argv[++i];
        else if (a == "--checkpoint-every") checkpointEvery = std::stoll(argv[++i]);
        else if (a == "--max-steps") maxSteps = std::stoll(argv[++i]);
        else if (a == "--resume") resumePath = argv[++i];
        else if (a == "--exact-film") exactFilm = true;
        else if (a == "--spp") mcSpp = std::stoi(argv[++i]);
        else if (a == "--max-spp") mcMaxSpp = std::stoi(argv[++i]);
        else if (a == "--film-layers") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            filmLayers = m == "length" ? 1 : m == "technique" ? 2 : 0;
            if (filmLayers == 0) {
                fprintf(stderr, "--film-layers: length or technique expected\n");
                return 2;
            }
        } else if (a == "--mc-layers") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            mcLayers = m == "length" ? 1 : m == "technique" ? 2 : 0;
            if (mcLayers == 0) {
                fprintf(stderr, "--mc-layers: length or technique expected\n");
                return 2;
            }
        }
        else if (a == "--trace-chains") traceChains = IntList(i + 1 < argc ? argv[++i] : ""), traceChainsGiven = true;
        else if (a == "--trace-file") traceFile = i + 1 < argc ? argv[++i] : "";
        else if (a == "--trace-steps") traceSteps = std::stoi(argv[++i]), traceStepsGiven = true;
        else if (a == "--step-table") stepTable = true;
        else filenames.push_back(a);
    }
    const bool wantTrace = traceChainsGiven || !traceFile.empty() || traceStepsGiven;
    if (wantTrace && (traceChains.empty() || traceFile.empty())) {
        fprintf(stderr, "--trace-chains a,b,.. and --trace-file FILE go together (--trace-steps S is optional)\n");
        return 2;
    }
    if (wantTrace && traceSteps <= 0) {
        fprintf(stderr, "--trace-steps: a positive number of steps expected\n");
        return 2;
    }
    if ((wantTrace || stepTable) && devices.size() > 1) {
        fprintf(stderr, "%s: chain diagnostics run on one device in this version (no --gpus / --devices list of more than one device)\n", wantTrace ? "--trace-chains" : "--step-table");
        return 2;
    }
    if (devices.empty()) devices.push_back(device);
    const int visible = lmc_device_count();
    for (int d : devices)
        if (d < 0 || d >= visible) {
            fprintf(stderr, "device %d requested, %d HIP device(s) visible\n", d, visible);
            return 2;
        }
    const int nDev = (int)devices.size();
    for (const std::string &filename : filenames) {
        std::vector<lmc_ctx *> ctxs;
        for (int d : devices) {
            lmc_scene_desc desc;
            memset(&desc, 0, sizeof(desc));
            desc.scene_xml = filename.c_str();
            desc.force_diffuse = forceDiffuse, desc.max_depth = maxDepth, desc.seed_offset = seedoffset, desc.device = d, desc.use_gradient = 1;
            lmc_ctx *c = lmc_create(&desc);
            if (!c) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            lmc_set_option(c, "max-derivatives-depth", maxDervDepth);
            ctxs.push_back(c);
        }
        lmc_ctx *ctx = ctxs[0];
        if (Opt(ctx, "integrator_mc") != 0) {  // main.cpp:92-96
            if (wantTrace || stepTable) {
                fprintf(stderr, "%s: %s has integrator=mc; only the Markov chains of an integrator=mcmc scene can be traced\n", wantTrace ? "--trace-chains" : "--step-table", filename.c_str());
                return 2;
            }
            if (filmLayers != 0) {
                fprintf(stderr, "--film-layers: %s has integrator=mc; its film is layered with --mc-layers\n", filename.c_str());
                return 2;
            }
            if (mltFlags) printf("--chains / --resident / --init-threads: ignored by integrator=mc\n");
            McFlags mf;
            mf.layers = mcLayers;
            mf.exactFilm = exactFilm, mf.spp = mcSpp, mf.maxSpp = mcMaxSpp, mf.checkpointPath = checkpointPath, mf.resumePath = resumePath;
            const int rc = RenderMC(filename, ctxs, mf);
            for (lmc_ctx *c : ctxs) lmc_destroy(c);
            if (rc != 0) return rc;
            printf("Done!\n");
            continue;
        }
        if (filmLayers != 0) {
            if (!checkpointPath.empty() || !resumePath.empty()) {
                fprintf(stderr, "--film-layers: a layered MLT film has no checkpoint in this version (no --checkpoint / --resume)\n");
                return 2;
            }
            exactFilm = true;
            for (lmc_ctx *c : ctxs)
                if (lmc_set_option(c, "film_layers", filmLayers) != 0) {
                    fprintf(stderr, "%s\n", lmc_last_error());
                    return 1;
                }
        }
        if (mcLayers != 0) {
            fprintf(stderr, "--mc-layers: %s has integrator=mcmc; only the film of an integrator=mc scene can be layered\n", filename.c_str());
            return 2;
        }
        if (Opt(ctx, "mala") == 0 && Opt(ctx, "h2mc") == 0) {
            fprintf(stderr, "dpt_amd serves the LMC path only (<dpt> integrator=mcmc with mala=true or h2mc=true)\n");
            return 1;
        }
        if (resident > 0 && Opt(ctx, "h2mc") != 0) printf("--resident: H2MC renders run in lock step\n");
        else if (resident > 0)
            for (lmc_ctx *c : ctxs)
                if (lmc_set_option(c, "resident_steps", resident) != 0) {
                    fprintf(stderr, "%s\n", lmc_last_error());
                    return 1;
                }
        int filmExact = exactFilm ? 1 : (int)Opt(ctx, "film_exact");  // (without the flag: the library's default, LMC_FILM_EXACT)
        if (!resumePath.empty()) {  // a resume takes the film's mode from the file
            char json[4096];
            if (lmc_checkpoint_info(resumePath.c_str(), json, sizeof(json)) < 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            const int fileExact = strstr(json, "\"film_format\":\"fixed64\"") != nullptr;
            if (exactFilm && !fileExact) {
                fprintf(stderr, "--exact-film: %s holds a float film; a render keeps the film mode it was started with\n", resumePath.c_str());
                return 2;
            }
            filmExact = fileExact;
        }
        for (lmc_ctx *c : ctxs)
            if (lmc_set_option(c, "film_exact", filmExact) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
        if (filmExact) printf("Exact film: 64-bit fixed-point accumulation\n");
        int info[8];
        lmc_info(ctx, info);
        const int W = info[0], H = info[1];
        const int spp = (int)Opt(ctx, "spp"), directSpp = (int)Opt(ctx, "directspp");
        const long long numChains = chains > 0 ? chains : (long long)Opt(ctx, "numchains");
        // mlt.cpp:33-47
        printf("Compute direct lighting\n");
        if (lmc_direct_lighting(ctx, directSpp) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        const long long totalSamples = (long long)spp * W * H;
        const long long numSamplesPerChain = totalSamples / numChains;
        const long long chainsNeedExtraSamples = numSamplesPerChain % numChains;  // (sic) mlt.cpp:40
        long long numInit = (long long)Opt(ctx, "numinitsamples");
        if (chains > 0 && numInit < 8 * numChains) {  // MLTInit needs at least as many contributions as chains (mlt.h:101-105)
            numInit = 8 * numChains;
            printf("numinitsamples raised to %lld for %lld chains\n", numInit, numChains);
        }
        if ((maxSteps >= 0 || checkpointEvery > 0) && checkpointPath.empty()) {
            fprintf(stderr, "--max-steps / --checkpoint-every need --checkpoint FILE\n");
            return 2;
        }
        auto saveCheckpoint = [&]() {
            if ((nDev == 1 ? lmc_checkpoint_save(ctx, checkpointPath.c_str()) : lmc_group_checkpoint_save(ctxs.data(), nDev, checkpointPath.c_str())) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                exit(1);
            }
        };
        long long stepsDone = 0;
        double secondsBefore = 0;
        if (nDev > 1) printf("%lld chains sharded over %d devices\n", numChains, nDev);
        if (!resumePath.empty()) {
            if ((nDev == 1 ? lmc_checkpoint_load(ctx, resumePath.c_str()) : lmc_group_checkpoint_load(ctxs.data(), nDev, resumePath.c_str())) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            char json[4096];
            if (lmc_checkpoint_info(resumePath.c_str(), json, sizeof(json)) < 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            stepsDone = (long long)JsonNumber(json, "steps_done"), secondsBefore = JsonNumber(json, "wall_seconds");
            if ((long long)JsonNumber(json, "n_chains_total") != numChains || (long long)JsonNumber(json, "samples_per_chain") != numSamplesPerChain) {
                fprintf(stderr, "%s holds %lld chains of %lld samples each, this run asks for %lld of %lld\n", resumePath.c_str(), (long long)JsonNumber(json, "n_chains_total"),
                        (long long)JsonNumber(json, "samples_per_chain"), numChains, numSamplesPerChain);
                return 1;
            }
            printf("Resumed %s: %lld steps, %g s so far\n", resumePath.c_str(), stepsDone, secondsBefore);
        } else if ((nDev == 1 ? lmc_chains_init(ctx, numInit, (int)numChains, initThreads, 0, (int)numChains, numSamplesPerChain, chainsNeedExtraSamples)
                       : lmc_group_chains_init(ctxs.data(), nDev, numInit, (int)numChains, initThreads, numSamplesPerChain, chainsNeedExtraSamples)) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        float normalization = 0;
        long long nContribs = 0;
        lmc_init_result(ctx, &normalization, &nContribs);
        printf("Average brightness:%g\n", normalization);
        if (wantTrace && lmc_chain_trace_begin(ctx, traceChains.data(), (int)traceChains.size(), traceSteps) != 0) {
            fprintf(stderr, "--trace-chains: %s\n", lmc_last_error());
            return 1;
        }
        if (stepTable && lmc_set_option(ctx, "step_table", 1) != 0) {
            fprintf(stderr, "--step-table: %s\n", lmc_last_error());
            return 1;
        }
        auto t0 = std::chrono::steady_clock::now();
        const long long targetSteps = (numSamplesPerChain + 1 + 63) / 64 * 64;  // calls of 64 steps; a chain that has run its samples is no longer stepped
        const long long stopAt = maxSteps >= 0 ? std::min(targetSteps, stepsDone + maxSteps) : targetSteps;
        while (stepsDone < stopAt) {
            long long n = std::min<long long>(64, stopAt - stepsDone);
            if (checkpointEvery > 0) n = std::min(n, checkpointEvery - stepsDone % checkpointEvery);
            if ((nDev == 1 ? lmc_chains_step(ctx, (int)n) : lmc_group_chains_step(ctxs.data(), nDev, (int)n)) != 0) {
                fprintf(stderr, "%s\n", lmc_last_error());
                return 1;
            }
            stepsDone += n;
            if (checkpointEvery > 0 && stepsDone % checkpointEvery == 0 && stepsDone < stopAt) saveCheckpoint();
        }
        for (lmc_ctx *c : ctxs) lmc_sync(c);
        if (!checkpointPath.empty()) {  // before the film merge: a merged film holds every member's share on every member
            saveCheckpoint();
            printf("Checkpoint after %lld of %lld steps: %s\n", stepsDone, targetSteps, checkpointPath.c_str());
        }
        if (nDev > 1 && lmc_group_film_reduce(ctxs.data(), nDev, nullptr) != 0) {  // the per-device films summed on the devices (peer copies); timed with the loop
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        const double elapsed = secondsBefore + std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();  // all legs of the render
        printf("Elapsed time:%g\n", elapsed);
        // MergeBuffer + BufferToFilm, mlt.cpp:203-207
        std::vector<float> direct((size_t)W * H * 3), indirect((size_t)W * H * 3), img((size_t)W * H * 3);
        lmc_direct_read(ctx, direct.data());
        lmc_film_read(ctx, indirect.data());
        const float dw = directSpp > 0 ? 1.0f / float(directSpp) : 0.0f, iw = spp > 0 ? 1.0f / float(spp) : 0.0f;
        for (size_t i = 0; i < img.size(); i++) img[i] = dw * direct[i] + iw * indirect[i];
        std::string dir = filename.rfind('/') != std::string::npos ? filename.substr(0, filename.rfind('/') + 1) : "";
        std::string out = dir + lmc_output_name(ctx) + "_timeuse_" + std::to_string(elapsed) + "s.exr";
        if (lmc_image_write_exr(out.c_str(), img.data(), W, H) != 0) {
            fprintf(stderr, "%s\n", lmc_last_error());
            return 1;
        }
        if (filmLayers != 0) {  // every non-empty layer beside the image, scaled as the indirect film above (after a merge every member holds the sums: member 0's)
            int mode = 0, nLayers = 0, written = 0;
            std::vector<int> cl(2 * 128);
            if (lmc_film_layer_info(ctx, &mode, &nLayers, cl.data(), 128) != 0 || nLayers > 128) {
                fprintf(stderr, "%s\n", nLayers > 128 ? "--film-layers: more than 128 layers" : lmc_last_error());
                return 1;
            }
            std::vector<float> layer((size_t)W * H * 3);
            for (int k = 0; k < nLayers; k++) {
                if (lmc_film_read_layer(ctx, k, layer.data()) != 0) {
                    fprintf(stderr, "%s\n", lmc_last_error());
                    return 1;
                }
                if (std::all_of(layer.begin(), layer.end(), [](float v) { return v == 0.0f; })) continue;
                for (float &v : layer) v = iw * v;
                char tag[64];
                if (mode == 1) snprintf(tag, sizeof(tag), "_L%02d", cl[2 * k]);
                else
                    snprintf(tag, sizeof(tag), "_c%d_l%d", cl[2 * k], cl[2 * k + 1]);
                const std::string name = out.substr(0, out.size() - 4) + tag + ".exr";
                if (lmc_image_write_exr(name.c_str(), layer.data(), W, H) != 0) {
                    fprintf(stderr, "%s\n", lmc_last_error());
                    return 1;
                }
                written++;
            }
            printf("Layered film (%s): %d of %d layers are non-empty and written beside the image\n", mode == 1 ? "by path length" : "by technique", written, nLayers);
        }
        long long mutations = 0, dropped = 0;
        for (lmc_ctx *c : ctxs) {
            long long st[8], ov = 0;
            double ws = 0;
            lmc_stats(c, st, &ws);
            mutations += st[0];
            lmc_film_overflow(c, &ov);
            dropped += ov;
        }
        if (dropped > 0) printf("Exact film: %lld splats with a component of 2^30 or more were dropped\n", dropped);
        printf("%lld mutations, %.1f M mutations/s, wrote %s\n", mutations, mutations / elapsed * 1e-6, out.c_str());
        if (wantTrace && WriteTrace(ctx, traceChains, traceSteps, traceFile) != 0) return 1;
        if (stepTable) {
            std::vector<long long> table(3 * 13 * 13 * 2);
            if (lmc_step_table(ctx, table.data(), 0) != 0) {
                fprintf(stderr, "--step-table: %s\n", lmc_last_error());
                return 1;
            }
            printf("Step table (kind: 1 large, 2 generic small, 3 lean small): kind c l steps accepted\n");
            for (int k = 0; k < 3; k++)
                for (int cc = 0; cc < 13; cc++)
                    for (int l = 0; l < 13; l++) {
                        const long long *cell = &table[(((size_t)k * 13 + cc) * 13 + l) * 2];
                        if (cell[0] || cell[1]) printf("%d %d %d %lld %lld\n", k + 1, cc, l, cell[0], cell[1]);
                    }
        }
        for (lmc_ctx *c : ctxs) lmc_destroy(c);
        printf("Done!\n");
    }
    return 0;
}
