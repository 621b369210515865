// fpmMain.cpp -- command-line drop-in for the reference's fpmMain
// (fpmMain.cpp:500-592):  `source use_gpu.sh; fpmMain <dataset.json> <itrCount>`
//
// Same JSON keys and defaults, same argv contract (argc < 3 prints usage and
// returns 0), same log lines ("Dataset Root: ...", "resImprovementFactor: N",
// "Loading Images...", "Loaded: <file>, LED # is: N", "Skipped LED# N",
// "Iteration i Completed (Time: t sec)", "FP Processing Completed (Time: t
// sec)").  The solver runs on the MI355X through libfpm_hip.so.  Instead of
// the reference's blocking showComplexImg windows (fpmMain.cpp:495-497) the
// results are written as .npy files: objCrop (L x L complex64), objF
// (un-centred spectrum), pupil (centred, Np x Np complex64), plus a
// result.json sidecar (geometry, LED order, iterations, timing).
//
// Extra options (after the two positional arguments):
//   --out DIR          output directory (default ".")
//   --device N         GPU ordinal (default 0)
//   --led-table FILE   "x y z" per line, metres or any unit, 1 row per LED:
//                      used when the JSON has no holeCoordinates (the
//                      reference aborts there; SURVEY.md 8(c) dome fallback)
//   --path general|fused|auto
//   --grid GXxGY       reconstruct a GX x GY field of patches instead of the
//                      reference's single crop: patch (i, j) is cut at
//                      (cropX + j*Np, cropY + i*Np) from every full frame on the
//                      GPU (fpm_upload_frames: the loader preprocessing of
//                      fpmMain.cpp:124-144 per patch), all patches are solved in
//                      one batch, and the stitched objCrop field
//                      (GY*Nlarge x GX*Nlarge complex64) is written as
//                      objCrop_field.npy with pupils.npy [B][Np][Np] (SURVEY.md
//                      8(f2)); result.json describes the grid
//   --overlap V        with --grid: neighbouring patches share V low-resolution
//                      pixels (0 <= V <= Np/2): patch (i, j) is cut at
//                      (cropX + j*(Np-V), cropY + i*(Np-V)), and the field is the
//                      tiles aligned and feathered on the GPU (fpm_stitch) at the
//                      stride (Np-V)*resImprovementFactor:
//                      ((GY-1)*stride + Nlarge) x ((GX-1)*stride + Nlarge).
//                      result.json gains "stitch": overlap, stride, align, field
//                      [H, W], factors [patches][2] (re, im), stitch_ms
//   --stitch-align none|phase|complex   with --overlap: bring every patch to its
//                      left and upper neighbours' phase (and, complex, scale) over
//                      the pixels they share before blending; default phase when
//                      V > 0
//   --write-tiles      also write objCrop_tiles.npy [patches][Nlarge][Nlarge]
//   --residual         report how well the state fits the data: fpm_residual
//                      after fpm_init and after every iteration (the iterations
//                      already run one fpm_run(ctx, 1) at a time, and a split run
//                      ends bit for bit where a single one does), written to
//                      result.json as "residual": per_iteration (itrCount + 1
//                      values of sum E / sum S over all patches and LEDs),
//                      per_patch_last, per_led_last (summed over patches, in
//                      processing order) and sweep_ms; with --grid the patches
//                      are the grid's; a figure whose S is 0 (all dark) is null.
//                      The .npy outputs do not change
//   --calibrate-leds R LED position calibration: after every iteration but the
//                      last, a window search of radius R (1 .. 8).  The residual
//                      of the current state is evaluated with every LED's
//                      window at each integer offset of the (2R+1)^2
//                      neighbourhood (fpm_residual_at, one batched sweep), summed
//                      over the patches; an LED moves to the candidate whose sum
//                      is strictly smaller than at its tabled position (ties: the
//                      nearest), and the corrected table replaces the live
//                      context's (fpm_set_crops).  result.json gains
//                      "led_calibration": radius, shift_total [used][2] (dx, dy
//                      in processing order), moved_per_iteration, crop_x0 /
//                      crop_y0 as used last, probe_ms.  Works with --grid and
//                      --residual (the sweep then follows the iteration and
//                      precedes the search)
//   --calibrate-gains  LED brightness calibration: after every iteration but the
//                      last, one gain step.  fpm_moments gives Q = sum |psi|^2,
//                      C = sum |psi| sqrt(I) and S = sum I of the current state
//                      per (LED, patch); the image's amplitude factor becomes
//                      g = C / S (unchanged where S = 0), each patch's factors
//                      are scaled to an S-weighted mean of g^2 of 1 (gain and
//                      object share a scale), clipped to [0.25, 4] and installed
//                      with fpm_set_gains: the solver then uses g sqrt(I)
//                      wherever it used sqrt(I).  result.json gains "led_gains":
//                      clip, gain [used][patches] as used last,
//                      before_per_step / after_per_step [steps][patches] (the
//                      patch sums of Q - 2 g C + g^2 S at the old and the new
//                      gains), moments_ms.  Combines with --calibrate-leds (the
//                      positions first) and --residual
//   --write-predicted amplitude|counts|diff   the forward model's images of the
//                      final state (fpm_predict), after the last iteration:
//                      predicted.npy [used][patches][Np][Np] in processing order,
//                      float32 |psi| (amplitude), uint16 rint((|psi| / g)^2)
//                      saturated at 65535, what the camera would record (counts),
//                      or float32 |psi| - g sqrt(I), the per-pixel mismatch with
//                      the measurements (diff); result.json gains "predicted":
//                      kind, shape, ms
//   --refocus Z0:DZ:N  digital refocusing of the final state (fpm_refocus): the
//                      field propagated to the N planes z = Z0 + k DZ by the
//                      angular-spectrum method, Z0 and DZ in the JSON's length
//                      unit (the one lambda and pixelSize use).  Every patch picks
//                      the plane where its focus measure is best, and
//                      objCrop_focus.npy [patches][Nlarge][Nlarge] holds every
//                      patch at its own plane.  result.json gains "refocus": z, zl
//                      (= z / lambda), fl (= lambda / (Nlarge ps)), margin,
//                      measure, pick, sum_a / sum_a2 / sum_g [N][patches] (the
//                      sums over the interior the measures are made of), plane
//                      and z_best [patches], ms.  With --grid, objCrop_field.npy
//                      is made of the focused tiles in place of objCrop: stitched
//                      on the device with --overlap (fpm_stitch_tiles), placed
//                      side by side without; objCrop_tiles.npy stays objCrop
//   --focus-measure nvar|tamura|grad   normalised variance (default), Tamura
//                      coefficient or gradient energy of the amplitude
//   --focus-pick max|min   the best plane has the largest (default) or the
//                      smallest value: min for phase objects, whose amplitude
//                      contrast is least in focus
//   --focus-margin PX  the sums leave out PX pixels along the border, where a
//                      propagated field wraps around (default 8, at most
//                      Nlarge/2 - 1)
//   --write-refocus    also write refocus.npy [N][patches][Nlarge][Nlarge]
//   --init-pupil FILE.npy  start from this pupil instead of the support disk:
//                      complex64 [Np][Np] (one pupil for every patch) or
//                      [patches][Np][Np], centred as pupil.npy / pupils.npy are
//                      written; the library keeps it on the support disk only
//   --init-objf FILE.npy   start from this spectrum: complex64 [Nlarge][Nlarge],
//                      un-centred as objF.npy is written; single-patch runs only,
//                      zero outside the band the used LEDs cover
//                      Both apply after fpm_init (fpm_set_state); with both
//                      given they apply instead of it, so objF.npy + pupil.npy
//                      of a run resume it.  The files (little-endian '<c8', C
//                      order, .npy version 1.0 or 2.0) are checked against the
//                      dataset's Np / Nlarge / --grid before the GPU is touched.
//                      result.json records what was used under "initial_state"
//
// Device selection: OPENCV_OPENCL_DEVICE (set by use_gpu.sh / use_cpu.sh) is
// read with OpenCV's "<platform>:<type>:<device>" grammar and the scripts'
// literal "GPU:0" / "CPU:0" form: a CPU type anywhere is refused (exit 3; the
// CPU restatement is the oracle, not a product path), a GPU index selects the
// MI355X ordinal; --device overrides it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/fpm_hip.h"
#include "../../include/fpm_host.h"

namespace {

bool write_npy_c64(const std::string &path, const float *data, int rows, int cols) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    char dict[128];
    snprintf(dict, sizeof dict, "{'descr': '<c8', 'fortran_order': False, 'shape': (%d, %d), }", rows, cols);
    std::string hdr = dict;
    size_t total = 10 + hdr.size() + 1;
    size_t pad = (64 - total % 64) % 64;
    hdr.append(pad, ' ');
    hdr.push_back('\n');
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    fwrite(magic, 1, 8, f);
    const unsigned short hl = (unsigned short)hdr.size();
    fwrite(&hl, 2, 1, f);
    fwrite(hdr.data(), 1, hdr.size(), f);
    fwrite(data, sizeof(float) * 2, (size_t)rows * cols, f);
    fclose(f);
    return true;
}

bool write_npy_c64_3d(const std::string &path, const float *data, int n0, int n1, int n2) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    char dict[128];
    snprintf(dict, sizeof dict, "{'descr': '<c8', 'fortran_order': False, 'shape': (%d, %d, %d), }", n0, n1, n2);
    std::string hdr = dict;
    size_t pad = (64 - (10 + hdr.size() + 1) % 64) % 64;
    hdr.append(pad, ' ');
    hdr.push_back('\n');
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    fwrite(magic, 1, 8, f);
    const unsigned short hl = (unsigned short)hdr.size();
    fwrite(&hl, 2, 1, f);
    fwrite(hdr.data(), 1, hdr.size(), f);
    fwrite(data, sizeof(float) * 2, (size_t)n0 * n1 * n2, f);
    return fclose(f) == 0;
}

// predicted.npy: float32 ('<f4') or uint16 ('<u2') [n0][n1][n2][n3]; refocus.npy: complex64 ('<c8')
bool write_npy_4d(const std::string &path, const void *data, const char *descr, size_t elem, int n0, int n1, int n2,
                  int n3) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    char dict[160];
    snprintf(dict, sizeof dict, "{'descr': '%s', 'fortran_order': False, 'shape': (%d, %d, %d, %d), }", descr, n0, n1,
             n2, n3);
    std::string hdr = dict;
    size_t pad = (64 - (10 + hdr.size() + 1) % 64) % 64;
    hdr.append(pad, ' ');
    hdr.push_back('\n');
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    fwrite(magic, 1, 8, f);
    const unsigned short hl = (unsigned short)hdr.size();
    fwrite(&hl, 2, 1, f);
    fwrite(hdr.data(), 1, hdr.size(), f);
    fwrite(data, elem, (size_t)n0 * n1 * n2 * n3, f);
    return fclose(f) == 0;
}

const char *kUsage =
    "Usage: fpmMain dataset.json itrCount [options]\n"
    "  --out DIR  --device N  --led-table FILE  --path general|fused|auto\n"
    "  --grid GXxGY  --overlap V  --stitch-align none|phase|complex  --write-tiles\n"
    "  --residual  --calibrate-leds R  --calibrate-gains\n"
    "  --init-pupil FILE.npy  --init-objf FILE.npy\n"
    "  --write-predicted amplitude|counts|diff\n"
    "      predicted.npy [used][patches][Np][Np]: the forward model's image of every LED for the\n"
    "      final state (float32 |psi|, uint16 counts, or float32 |psi| - g sqrt(I))\n"
    "  --refocus Z0:DZ:N  --focus-measure nvar|tamura|grad  --focus-pick max|min  --focus-margin PX\n"
    "  --write-refocus\n"
    "      the final field propagated to the planes z = Z0 + k DZ (the JSON's length unit); every\n"
    "      patch at the plane its focus measure picks: objCrop_focus.npy [patches][Nlarge][Nlarge];\n"
    "      --write-refocus: every plane, refocus.npy [N][patches][Nlarge][Nlarge]; with --grid the\n"
    "      field is made of the focused tiles (stitched with --overlap, placed side by side without)\n";

// A .npy file of little-endian complex64 in C order, format version 1.0 or
// 2.0: its shape and its values as (re, im) pairs.  The header's shape must
// be one of `accepted` (what the dataset allows; `layout` names them in the
// message) before a value is read or a byte allocated for it.  Anything else
// is an error whose text names the file.
struct NpyC64 {
    std::vector<int64_t> shape;
    std::vector<float> data;
};
std::string shape_text(const std::vector<int64_t> &s) {
    std::string t = "(";
    for (size_t i = 0; i < s.size(); ++i) t += (i ? ", " : "") + std::to_string(s[i]);
    return t + ")";
}
bool read_npy_c64(const std::string &path, const std::vector<std::vector<int64_t>> &accepted, const char *layout,
                  NpyC64 *out, std::string *err) {
    auto fail = [&](const std::string &why) {
        *err = path + ": " + why;
        return false;
    };
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail("cannot open");
    unsigned char pre[12];
    if (!f.read((char *)pre, 8) || std::memcmp(pre, "\x93NUMPY", 6) != 0) return fail("not a .npy file");
    const int major = pre[6];
    if (major != 1 && major != 2) return fail("unsupported .npy version " + std::to_string(major) + " (1.0 or 2.0)");
    const int nlen = major == 1 ? 2 : 4;
    if (!f.read((char *)pre + 8, nlen)) return fail("truncated header");
    size_t hl = 0;
    for (int i = 0; i < nlen; ++i) hl |= (size_t)pre[8 + i] << (8 * i);
    if (hl > (1u << 20)) return fail("header too long");
    std::string hdr(hl, '\0');
    if (!f.read(&hdr[0], (std::streamsize)hl)) return fail("truncated header");
    // the value that follows 'key': up to the next comma outside parentheses
    auto value = [&](const char *key) {
        size_t p = hdr.find(std::string("'") + key + "'");
        if (p == std::string::npos) return std::string();
        p = hdr.find(':', p);
        if (p == std::string::npos) return std::string();
        size_t q = ++p;
        for (int depth = 0; q < hdr.size(); ++q) {
            if (hdr[q] == '(') ++depth;
            if (hdr[q] == ')') --depth;
            if ((hdr[q] == ',' && depth == 0) || hdr[q] == '}') break;
        }
        std::string v = hdr.substr(p, q - p);
        const size_t a = v.find_first_not_of(" "), b = v.find_last_not_of(" ");
        return a == std::string::npos ? std::string() : v.substr(a, b - a + 1);
    };
    const std::string descr = value("descr"), forder = value("fortran_order"), shape = value("shape");
    if (descr != "'<c8'" && descr != "\"<c8\"") return fail("dtype " + descr + ", want '<c8' (little-endian complex64)");
    if (forder != "False") return fail("Fortran order, want C order");
    if (shape.size() < 2 || shape.front() != '(' || shape.back() != ')') return fail("unreadable shape " + shape);
    out->shape.clear();
    for (size_t p = 1; p < shape.size() - 1;) {
        const size_t q = std::min(shape.find(',', p), shape.size() - 1);
        const std::string t = shape.substr(p, q - p);
        if (t.find_first_not_of(" ") != std::string::npos) {
            char *end = nullptr;
            const long long v = strtoll(t.c_str(), &end, 10);
            while (*end == ' ') ++end;
            if (*end || v < 0 || v > (1ll << 31)) return fail("unreadable shape " + shape);
            out->shape.push_back(v);
        }
        p = q + 1;
    }
    if (std::find(accepted.begin(), accepted.end(), out->shape) == accepted.end()) {
        std::string want;
        for (size_t i = 0; i < accepted.size(); ++i) want += (i ? " or " : "") + shape_text(accepted[i]);
        return fail("shape " + shape_text(out->shape) + ", expected " + want + " (" + layout + ")");
    }
    size_t count = 1;  // of an accepted shape: the dataset's sizes
    for (int64_t v : out->shape) count *= (size_t)v;
    out->data.resize(count * 2);
    if (!f.read((char *)out->data.data(), (std::streamsize)(count * 2 * sizeof(float))))
        return fail("fewer values than its shape " + shape);
    return true;
}

// OPENCV_OPENCL_DEVICE -> (refuse CPU, GPU ordinal).  OpenCV splits the value
// at ':' into platform, device type(s) ('|'-separated) and device name/index;
// use_gpu.sh / use_cpu.sh write "GPU:0" / "CPU:0" (type first).  Returns 3
// for a CPU selection, else 0 and sets *ordinal when an index is given.
int parse_opencl_device(const char *v, int *ordinal) {
    std::vector<std::string> parts;
    std::string cur;
    for (const char *c = v; *c; ++c) {
        if (*c == ':') {
            parts.push_back(cur);
            cur.clear();
        } else {
            cur.push_back((char)toupper((unsigned char)*c));
        }
    }
    parts.push_back(cur);
    auto has_type = [](const std::string &field, const char *t) {
        size_t p = 0;
        while (p <= field.size()) {
            size_t q = field.find('|', p);
            if (q == std::string::npos) q = field.size();
            if (field.compare(p, q - p, t) == 0) return true;
            p = q + 1;
        }
        return false;
    };
    for (size_t i = 0; i < parts.size() && i < 2; ++i)
        if (has_type(parts[i], "CPU")) return 3;
    auto is_num = [](const std::string &x) { return !x.empty() && x.find_first_not_of("0123456789") == std::string::npos; };
    if (parts.size() == 2 && has_type(parts[0], "GPU") && is_num(parts[1])) *ordinal = atoi(parts[1].c_str());
    else if (parts.size() == 3 && is_num(parts[2])) *ordinal = atoi(parts[2].c_str());
    return 0;
}

bool read_led_table(const std::string &path, std::vector<float> *xyz) {
    std::ifstream f(path);
    if (!f) return false;
    float a, b, c;
    while (f >> a >> b >> c) {
        xyz->push_back(a);
        xyz->push_back(b);
        xyz->push_back(c);
    }
    return !xyz->empty();
}

}  // namespace

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--help") {
            std::cout << kUsage;
            return 0;
        }
    if (argc < 3) {
        std::cout << "ERROR: Not enough input argumants.\n Usage: ./fpmMain dataset.json" << std::endl;
        return 0;
    }
    std::string out_dir = ".", led_table, path_opt = "auto", init_pupil, init_objf;
    int device = 0, device_opt = -1, gx = 0, gy = 0;
    bool want_residual = false;
    bool want_gains = false;  // --calibrate-gains: one gain step between the iterations
    int cal_radius = -1;  // --calibrate-leds R: a window search of radius R between the iterations
    int overlap = -1;          // --overlap V: low-resolution pixels neighbouring patches share (-1: not given)
    std::string stitch_align;  // --stitch-align none|phase|complex
    bool write_tiles = false;  // --write-tiles: objCrop_tiles.npy [B][L][L] as well
    std::string predicted;     // --write-predicted amplitude|counts|diff: predicted.npy of the final state
    int rf_n = 0;              // --refocus Z0:DZ:N: planes z = Z0 + k DZ (0: not given)
    double rf_z0 = 0, rf_dz = 0;
    std::string focus_measure = "nvar", focus_pick = "max";  // --focus-measure, --focus-pick
    int focus_margin = -1;     // --focus-margin PX (-1: the default)
    bool write_refocus = false, focus_opt = false;  // --write-refocus; some --focus-* option was given
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--out" && i + 1 < argc) out_dir = argv[++i];
        else if (a == "--write-tiles") write_tiles = true;
        else if (a == "--overlap" && i + 1 < argc) {
            char *end = nullptr;
            const long v = strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > (1 << 20)) {
                std::cerr << "--overlap wants a number of pixels >= 0" << std::endl;
                return 2;
            }
            overlap = (int)v;
        }
        else if (a == "--stitch-align" && i + 1 < argc) {
            stitch_align = argv[++i];
            if (stitch_align != "none" && stitch_align != "phase" && stitch_align != "complex") {
                std::cerr << "--stitch-align wants none, phase or complex" << std::endl;
                return 2;
            }
        }
        else if (a == "--device" && i + 1 < argc) device_opt = atoi(argv[++i]);
        else if (a == "--led-table" && i + 1 < argc) led_table = argv[++i];
        else if (a == "--path" && i + 1 < argc) path_opt = argv[++i];
        else if (a == "--init-pupil" && i + 1 < argc) init_pupil = argv[++i];
        else if (a == "--init-objf" && i + 1 < argc) init_objf = argv[++i];
        else if (a == "--residual") want_residual = true;
        else if (a == "--write-predicted" && i + 1 < argc) {
            predicted = argv[++i];
            if (predicted != "amplitude" && predicted != "counts" && predicted != "diff") {
                std::cerr << "--write-predicted wants amplitude, counts or diff" << std::endl;
                return 2;
            }
        }
        else if (a == "--refocus" && i + 1 < argc) {
            char tail = 0;
            if (sscanf(argv[++i], "%lf:%lf:%d%c", &rf_z0, &rf_dz, &rf_n, &tail) != 3 || !std::isfinite(rf_z0) ||
                !std::isfinite(rf_dz) || rf_n < 1 || rf_n > 4096) {
                std::cerr << "--refocus wants Z0:DZ:N, e.g. -20:5:9 (N planes from 1 to 4096)" << std::endl;
                return 2;
            }
        }
        else if (a == "--focus-measure" && i + 1 < argc) {
            focus_measure = argv[++i];
            focus_opt = true;
            if (focus_measure != "nvar" && focus_measure != "tamura" && focus_measure != "grad") {
                std::cerr << "--focus-measure wants nvar, tamura or grad" << std::endl;
                return 2;
            }
        }
        else if (a == "--focus-pick" && i + 1 < argc) {
            focus_pick = argv[++i];
            focus_opt = true;
            if (focus_pick != "max" && focus_pick != "min") {
                std::cerr << "--focus-pick wants max or min" << std::endl;
                return 2;
            }
        }
        else if (a == "--focus-margin" && i + 1 < argc) {
            char *end = nullptr;
            const long v = strtol(argv[++i], &end, 10);
            focus_opt = true;
            if (end == argv[i] || *end || v < 0 || v > (1 << 20)) {
                std::cerr << "--focus-margin wants a number of pixels >= 0" << std::endl;
                return 2;
            }
            focus_margin = (int)v;
        }
        else if (a == "--write-refocus") write_refocus = true;
        else if (a == "--calibrate-gains") want_gains = true;
        else if (a == "--calibrate-leds" && i + 1 < argc) {
            cal_radius = atoi(argv[++i]);
            if (cal_radius < 1 || cal_radius > 8) {
                std::cerr << "--calibrate-leds wants a radius from 1 to 8" << std::endl;
                return 2;
            }
        }
        else if (a == "--grid" && i + 1 < argc) {
            if (sscanf(argv[++i], "%dx%d", &gx, &gy) != 2 || gx < 1 || gy < 1) {
                std::cerr << "--grid wants GXxGY, e.g. 16x16" << std::endl;
                return 2;
            }
        } else {
            std::cerr << "unknown option " << a << std::endl;
            return 2;
        }
    }
    if (overlap >= 0 && gx < 1) {
        std::cerr << "--overlap needs --grid: it is the overlap of the grid's neighbouring patches" << std::endl;
        return 2;
    }
    if (!stitch_align.empty() && overlap < 0) {
        std::cerr << "--stitch-align needs --overlap: without it the tiles share no pixels to align on" << std::endl;
        return 2;
    }
    if ((write_refocus || focus_opt) && rf_n < 1) {
        std::cerr << "--write-refocus and --focus-* need --refocus Z0:DZ:N: they describe its planes" << std::endl;
        return 2;
    }
    // use_cpu.sh / use_gpu.sh select the OpenCL device (use_gpu.sh:1)
    const char *dev = getenv("OPENCV_OPENCL_DEVICE");
    if (dev && *dev) {
        if (parse_opencl_device(dev, &device) == 3) {
            std::cerr << "OPENCV_OPENCL_DEVICE=" << dev
                      << ": this build runs the solver on MI355X only (source use_gpu.sh). The CPU "
                         "restatement of runFPM lives in oracle/ and is a test checker, not a product path."
                      << std::endl;
            return 3;
        }
    }
    if (device_opt >= 0) device = device_opt;
    std::cout << "Device: MI355X ordinal " << device << std::endl;

    fpm_host *h = nullptr;
    if (fpm_host_open(argv[1], &h)) {
        std::cerr << fpm_host_last_error() << std::endl;
        return 1;
    }
    fpm_host_config cfg;
    fpm_host_get_config(h, &cfg);
    const int itr_count = atoi(argv[2]);  // fpmMain.cpp:569
    std::cout << "Dataset Root: " << cfg.dataset_root << std::endl;
    std::cout << "resImprovementFactor: " << cfg.res_improvement_factor << std::endl;
    if (overlap > cfg.np / 2) {
        std::cerr << "--overlap " << overlap << " exceeds Np/2 = " << cfg.np / 2
                  << ": a pixel may lie in at most two patches per axis" << std::endl;
        return 2;
    }
    if (rf_n > 0) {
        if (focus_margin < 0) focus_margin = std::min(8, (cfg.nlarge - 2) / 2);
        if (2 * focus_margin > cfg.nlarge - 2) {
            std::cerr << "--focus-margin " << focus_margin << " leaves no interior: at most " << (cfg.nlarge - 2) / 2
                      << " for Nlarge " << cfg.nlarge << std::endl;
            return 2;
        }
        if (!(cfg.lambda > 0) || !(cfg.ps > 0)) {
            std::cerr << "--refocus needs lambda and pixelSize > 0 in the dataset JSON" << std::endl;
            return 2;
        }
    }
    if (overlap > 0 && stitch_align.empty()) stitch_align = "phase";
    if (overlap == 0 && stitch_align.empty()) stitch_align = "none";
    // --init-pupil / --init-objf: read and checked against the dataset before
    // anything is loaded or the GPU is touched
    NpyC64 pupil0, objf0;
    bool pupil0_shared = false;
    {
        const int64_t n = cfg.np, l = cfg.nlarge, nb = gx > 0 ? gx * gy : 1;
        std::string err;
        if (!init_pupil.empty()) {
            if (!read_npy_c64(init_pupil, {{n, n}, {nb, n, n}}, "[Np][Np] or [patches][Np][Np]", &pupil0, &err)) {
                std::cerr << "--init-pupil " << err << std::endl;
                return 2;
            }
            pupil0_shared = pupil0.shape.size() == 2;
        }
        if (!init_objf.empty()) {
            if (nb != 1) {
                std::cerr << "--init-objf " << init_objf << ": single-patch runs only (not with --grid)" << std::endl;
                return 2;
            }
            if (!read_npy_c64(init_objf, {{l, l}}, "[Nlarge][Nlarge]", &objf0, &err)) {
                std::cerr << "--init-objf " << err << std::endl;
                return 2;
            }
        }
    }
    if (!led_table.empty()) {
        std::vector<float> xyz;
        if (!read_led_table(led_table, &xyz)) {
            std::cerr << "cannot read LED table " << led_table << std::endl;
            return 1;
        }
        fpm_host_set_led_table(h, xyz.data(), (int)(xyz.size() / 3));
    }
    std::cout << "Loading Images..." << std::endl;
    if (fpm_host_scan(h) < 0) {
        std::cout << "ERROR: Could not Open Directory." << std::endl;
        return 1;
    }
    const int used = fpm_host_geometry(h);
    if (used <= 0) {
        std::cout << fpm_host_last_error() << std::endl;
        return 1;
    }
    std::vector<fpm_host_led> leds(fpm_host_n_present(h));
    fpm_host_get_leds(h, leds.data(), (int)leds.size());
    for (auto &l : leds) {
        std::cout << "NA:" << l.illumination_na << std::endl;
        if (!l.used) std::cout << "Skipped LED# " << l.led << std::endl;
    }
    const int np = cfg.np, L = cfg.nlarge;
    const bool grid = gx > 0;
    const int B = grid ? gx * gy : 1;
    std::vector<int32_t> order(used), x0(used), y0(used);
    fpm_host_get_order(h, order.data(), used);
    fpm_host_get_crops(h, x0.data(), y0.data(), used);
    std::vector<uint16_t> stack, frames;
    int32_t fw = 0, fh = 0;
    if (!grid) {
        if (fpm_host_load_images(h) < 0) {
            std::cerr << fpm_host_last_error() << std::endl;
            return 1;
        }
        stack.resize((size_t)used * np * np);
        fpm_host_get_stack(h, stack.data(), stack.size());
    } else {
        if (fpm_host_load_frames(h, nullptr, 0, &fw, &fh) < 0) {
            std::cerr << fpm_host_last_error() << std::endl;
            return 1;
        }
        frames.resize((size_t)used * fw * fh);
        if (fpm_host_load_frames(h, frames.data(), frames.size(), nullptr, nullptr) < 0) {
            std::cerr << fpm_host_last_error() << std::endl;
            return 1;
        }
    }
    for (int i = 0; i < used; ++i) std::cout << "Loaded: LED # is: " << order[i] << std::endl;

    std::vector<int32_t> ident(used);
    for (int i = 0; i < used; ++i) ident[i] = i;  // stack index i == sortedIndicies[i]
    fpm_problem p;
    std::memset(&p, 0, sizeof p);
    p.np = np;
    p.nlarge = L;
    p.n_stack = used;
    p.n_order = used;
    p.order = ident.data();
    p.crop_x0 = x0.data();
    p.crop_y0 = y0.data();
    p.na_radius = cfg.na_radius;
    p.init_pos = 1;
    p.delta1 = cfg.delta1;
    p.delta2 = cfg.delta2;
    p.eps = (double)1e-10f;
    p.n_patch = B;
    p.path = path_opt == "general" ? FPM_PATH_GENERAL : path_opt == "fused" ? FPM_PATH_FUSED : FPM_PATH_AUTO;
    fpm_ctx *ctx = nullptr;
    int rc = fpm_create(&p, device, &ctx);
    std::vector<int16_t> bg(used, 0);
    if (!rc && !grid) rc = fpm_upload_stack(ctx, stack.data());
    if (!rc && grid) {
        // patch (i, j) of the field at (cropX + j step, cropY + i step), step = Np
        // less --overlap; the darkfield divide applies where illumination NA >
        // objective NA (:128)
        const int step = np - std::max(overlap, 0);
        std::vector<int32_t> px(B), py(B);
        for (int i = 0; i < gy; ++i)
            for (int j = 0; j < gx; ++j) {
                px[i * gx + j] = cfg.crop_x + j * step;
                py[i * gx + j] = cfg.crop_y + i * step;
            }
        std::vector<fpm_host_led> all(fpm_host_n_present(h));
        fpm_host_get_leds(h, all.data(), (int)all.size());
        std::vector<uint8_t> dark(used, 0);
        for (int s2 = 0; s2 < used; ++s2)
            for (auto &l : all)
                if (l.led == order[s2]) dark[s2] = l.illumination_na > cfg.objective_na;
        fpm_frames fr;
        std::memset(&fr, 0, sizeof fr);
        fr.height = fh;
        fr.width = fw;
        fr.patch_x0 = px.data();
        fr.patch_y0 = py.data();
        fr.bk1_x = cfg.bk1_crop_x;
        fr.bk1_y = cfg.bk1_crop_y;
        fr.bk2_x = cfg.bk2_crop_x;
        fr.bk2_y = cfg.bk2_crop_y;
        fr.bg_threshold = cfg.bg_threshold;
        fr.darkfield_exp_multiplier = cfg.darkfield_exp_multiplier;
        fr.darkfield = dark.data();
        rc = fpm_upload_frames(ctx, &fr, frames.data(), 0, bg.data());
        frames.clear();
        frames.shrink_to_fit();
    }
    // a given pupil / spectrum replaces fpm_init's after it; both together replace it
    const bool have_pupil0 = !init_pupil.empty(), have_objf0 = !init_objf.empty();
    if (!rc && !(have_pupil0 && have_objf0)) rc = fpm_init(ctx);
    if (!rc && (have_pupil0 || have_objf0))
        rc = fpm_set_state(ctx, have_objf0 ? objf0.data.data() : nullptr, have_pupil0 ? pupil0.data.data() : nullptr,
                           pupil0_shared ? FPM_STATE_PUPIL_SHARED : 0u);
    if (rc) {
        std::cerr << "fpm: " << fpm_last_error() << std::endl;
        return 1;
    }
    // --residual: E and S [used][B] of the latest sweep, and their sums over
    // everything after fpm_init and after each iteration
    std::vector<double> res_e, res_s, res_iter_e, res_iter_s;
    double res_ms = 0;
    auto residual = [&]() {
        res_e.resize((size_t)used * B);
        res_s.resize((size_t)used * B);
        if (fpm_residual(ctx, res_e.data(), res_s.data(), &res_ms)) return false;
        double e = 0, s = 0;
        for (size_t i = 0; i < res_e.size(); ++i) {
            e += res_e[i];
            s += res_s[i];
        }
        res_iter_e.push_back(e);
        res_iter_s.push_back(s);
        return true;
    };
    // sum E / sum S as JSON; null where every pixel summed is dark (S = 0)
    auto put_ratio = [](FILE *f, const char *sep, double e, double s) {
        if (s > 0) fprintf(f, "%s%.17g", sep, e / s);
        else fprintf(f, "%snull", sep);
    };
    if (want_residual && !residual()) {
        std::cerr << "fpm: " << fpm_last_error() << std::endl;
        return 1;
    }
    // --calibrate-leds R: one search step after every iteration but the last.
    // Every LED's E, summed over the patches, with its window at each offset
    // of the (2R+1)^2 neighbourhood ((0, 0) first, then by growing distance);
    // an LED moves to the first candidate whose sum is strictly smaller than at
    // (0, 0); the corrected table goes to the live context (fpm_set_crops).
    std::vector<int32_t> cal_x = x0, cal_y = y0, cal_moved;
    double cal_ms = 0;
    std::vector<std::pair<int, int>> cal_offs;
    for (int dy = -cal_radius; dy <= cal_radius; ++dy)
        for (int dx = -cal_radius; dx <= cal_radius; ++dx) cal_offs.push_back({dx, dy});
    std::stable_sort(cal_offs.begin(), cal_offs.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) {
        return a.first * a.first + a.second * a.second < b.first * b.first + b.second * b.second;
    });
    auto calibrate = [&]() {
        std::vector<fpm_probe> probes;  // LED-major: an LED's candidates are adjacent
        for (int i = 0; i < used; ++i)
            for (auto &o : cal_offs) {
                const int x = cal_x[i] + o.first, y = cal_y[i] + o.second;
                if (x >= 0 && x <= L - np && y >= 0 && y <= L - np) probes.push_back({i, o.first, o.second});
            }
        std::vector<double> e(probes.size() * (size_t)B);
        double ms = 0;
        if (fpm_residual_at(ctx, probes.data(), (int)probes.size(), e.data(), nullptr, &ms)) return false;
        cal_ms += ms;
        int moved = 0;
        for (size_t k = 0, end; k < probes.size(); k = end) {
            const int i = probes[k].pos;  // its entries are [k, end), (0, 0) first
            double best = 0;
            size_t at = k;
            for (end = k; end < probes.size() && probes[end].pos == i; ++end) {
                double sum = 0;
                for (int b = 0; b < B; ++b) sum += e[end * B + b];
                if (end == k || sum < best) best = sum, at = end;
            }
            cal_x[i] += probes[at].dx;
            cal_y[i] += probes[at].dy;
            moved += probes[at].dx != 0 || probes[at].dy != 0;
        }
        cal_moved.push_back(moved);
        return moved == 0 || fpm_set_crops(ctx, cal_x.data(), cal_y.data()) == 0;
    };
    // --calibrate-gains: one estimate-and-apply step after every iteration but
    // the last (fpm_amd.calibrate.estimate_gains' rule; stack index i == position i)
    const double gain_lo = 0.25, gain_hi = 4.0;
    std::vector<float> gain((size_t)used * B, 1.0f);
    std::vector<std::vector<double>> gain_before, gain_after;  // [step][patch]
    double gain_ms = 0;
    auto calibrate_gains = [&]() {
        const size_t n = (size_t)used * B;
        std::vector<double> q(n), c(n), s(n);
        double ms = 0;
        if (fpm_moments(ctx, nullptr, 0, q.data(), c.data(), s.data(), &ms)) return false;
        gain_ms += ms;
        std::vector<float> next = gain;
        std::vector<double> before(B, 0.0), after(B, 0.0);
        for (int b = 0; b < B; ++b) {
            double sw = 0, swg = 0;
            for (int i = 0; i < used; ++i) {
                const size_t k = (size_t)i * B + b;
                if (!(s[k] > 0)) continue;
                const double g = c[k] / s[k];
                sw += s[k];
                swg += s[k] * g * g;
            }
            const double scale = swg > 0 ? std::sqrt(sw / swg) : 0.0;
            for (int i = 0; i < used; ++i) {
                const size_t k = (size_t)i * B + b;
                if (s[k] > 0 && swg > 0)
                    next[k] = (float)std::min(gain_hi, std::max(gain_lo, c[k] / s[k] * scale));
                const double g0 = gain[k], g1 = next[k];
                before[b] += q[k] - 2 * g0 * c[k] + g0 * g0 * s[k];
                after[b] += q[k] - 2 * g1 * c[k] + g1 * g1 * s[k];
            }
        }
        gain_before.push_back(before);
        gain_after.push_back(after);
        if (fpm_set_gains(ctx, next.data())) return false;
        gain.swap(next);
        return true;
    };
    auto t_all = std::chrono::steady_clock::now();
    for (int itr = 1; itr <= itr_count; ++itr) {
        auto t0 = std::chrono::steady_clock::now();
        if ((rc = fpm_run(ctx, 1)) || (want_residual && !residual()) ||
            (cal_radius > 0 && itr < itr_count && !calibrate()) ||
            (want_gains && itr < itr_count && !calibrate_gains())) {
            std::cerr << "fpm: " << fpm_last_error() << std::endl;
            return 1;
        }
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "Iteration " << itr << " Completed (Time: " << dt << " sec)" << std::endl;
    }
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
    std::cout << "FP Processing Completed (Time: " << dt << " sec)" << std::endl;

    std::vector<float> objF(grid ? 0 : (size_t)L * L * 2), objCrop((size_t)B * L * L * 2),
        pupil((size_t)B * np * np * 2);
    if ((rc = fpm_download(ctx, grid ? nullptr : objF.data(), objCrop.data(), pupil.data(), nullptr))) {
        std::cerr << "fpm: " << fpm_last_error() << std::endl;
        return 1;
    }
    // --overlap: the field is the tiles aligned and blended on the GPU (fpm_stitch)
    const bool blend = grid && overlap >= 0;
    const int st_stride = (np - std::max(overlap, 0)) * (L / np);  // Nlarge = Np * resImprovementFactor
    const int st_h = (gy - 1) * st_stride + L, st_w = (gx - 1) * st_stride + L;
    std::vector<float> st_field;
    std::vector<double> st_factors;
    double st_ms = 0;
    const fpm_stitch_grid sg = {gy, gx, L, st_stride, st_stride};
    const uint32_t sflags = stitch_align == "phase"     ? FPM_STITCH_ALIGN_PHASE
                            : stitch_align == "complex" ? FPM_STITCH_ALIGN_COMPLEX
                                                        : 0u;
    if (blend) {
        st_field.resize((size_t)st_h * st_w * 2);
        st_factors.resize((size_t)B * 2);
    }
    // --refocus: the sweep (sums, and every plane with --write-refocus), the
    // host's choice of a plane per patch, then every patch at its own z from one
    // per-patch call.  With --overlap that call stores into device memory and the
    // focused tiles are stitched where they lie (fpm_stitch_tiles).
    const size_t tile_f = (size_t)L * L * 2;
    std::vector<double> rf_z(rf_n), rf_zl(rf_n), rf_sa, rf_sa2, rf_sg, rf_zbest(B);
    std::vector<int> rf_plane(B, 0);
    std::vector<float> rf_all, rf_focus;
    const double rf_fl = rf_n > 0 ? (double)cfg.lambda / ((double)L * (double)cfg.ps) : 0.0;
    double rf_ms = 0;
    if (rf_n > 0) {
        const size_t nb = (size_t)rf_n * B;
        for (int k = 0; k < rf_n; ++k) {
            rf_z[k] = rf_z0 + k * rf_dz;
            rf_zl[k] = rf_z[k] / (double)cfg.lambda;
        }
        rf_sa.resize(nb);
        rf_sa2.resize(nb);
        rf_sg.resize(nb);
        if (write_refocus) rf_all.resize(nb * tile_f);
        double ms = 0;
        if ((rc = fpm_refocus(ctx, rf_zl.data(), rf_n, rf_fl, focus_margin, 0u, write_refocus ? rf_all.data() : nullptr,
                              rf_sa.data(), rf_sa2.data(), rf_sg.data(), &ms))) {
            std::cerr << "fpm: " << fpm_last_error() << std::endl;
            return 1;
        }
        rf_ms += ms;
        // N = |R|, m = sum_a / N, v = sum_a2 / N - m^2: v / m^2, sqrt(sqrt(v) / m), sum_g / sum_a2
        const double N = (double)(L - 2 * focus_margin) * (L - 2 * focus_margin);
        auto measure = [&](size_t k) {
            const double m = rf_sa[k] / N, v = std::max(rf_sa2[k] / N - m * m, 0.0);
            return focus_measure == "nvar" ? v / (m * m) : focus_measure == "tamura" ? std::sqrt(std::sqrt(v) / m)
                                                                                     : rf_sg[k] / rf_sa2[k];
        };
        std::vector<double> zlb(B);
        for (int b = 0; b < B; ++b) {
            for (int k = 1; k < rf_n; ++k) {  // the first of equal values
                const double v = measure((size_t)k * B + b), best = measure((size_t)rf_plane[b] * B + b);
                if (focus_pick == "max" ? v > best : v < best) rf_plane[b] = k;
            }
            rf_zbest[b] = rf_z[rf_plane[b]];
            zlb[b] = rf_zl[rf_plane[b]];
        }
        rf_focus.resize((size_t)B * tile_f);
        if (!blend) {
            rc = fpm_refocus(ctx, zlb.data(), 1, rf_fl, focus_margin, FPM_REFOCUS_Z_PER_PATCH, rf_focus.data(), nullptr,
                             nullptr, nullptr, &ms);
        } else {
            struct Dev {
                void *p = nullptr;
                ~Dev() { (void)hipFree(p); }
            } tiles, field;
            const size_t tb = (size_t)B * tile_f * sizeof(float), fb = st_field.size() * sizeof(float);
            if (hipSetDevice(device) != hipSuccess || hipMalloc(&tiles.p, tb) != hipSuccess || hipMalloc(&field.p, fb) != hipSuccess) {
                std::cerr << "--refocus: no device memory for the focused tiles and the field" << std::endl;
                return 1;
            }
            rc = fpm_refocus(ctx, zlb.data(), 1, rf_fl, focus_margin, FPM_REFOCUS_Z_PER_PATCH | FPM_REFOCUS_DEVICE,
                             (float *)tiles.p, nullptr, nullptr, nullptr, &ms);
            if (!rc)
                rc = fpm_stitch_tiles(device, (const float *)tiles.p, &sg, sflags | FPM_STITCH_DEVICE, (float *)field.p,
                                      st_factors.data(), nullptr, &st_ms);
            if (!rc && (hipMemcpy(rf_focus.data(), tiles.p, tb, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(st_field.data(), field.p, fb, hipMemcpyDeviceToHost) != hipSuccess)) {
                std::cerr << "--refocus: copying the focused tiles and the field back failed" << std::endl;
                return 1;
            }
        }
        if (rc) {
            std::cerr << "fpm: " << fpm_last_error() << std::endl;
            return 1;
        }
        rf_ms += ms;
    } else if (blend) {
        if ((rc = fpm_stitch(ctx, &sg, sflags, st_field.data(), st_factors.data(), &st_ms))) {
            std::cerr << "fpm: " << fpm_last_error() << std::endl;
            return 1;
        }
    }
    // --write-predicted: the forward model's images of the final state (fpm_predict)
    std::vector<uint32_t> pred;  // float32, or uint16 in the leading half
    double pred_ms = 0;
    if (!predicted.empty()) {
        const uint32_t kind = predicted == "counts" ? FPM_PREDICT_COUNTS
                              : predicted == "diff" ? FPM_PREDICT_DIFF
                                                    : FPM_PREDICT_AMPLITUDE;
        pred.resize((size_t)used * B * np * np);
        if ((rc = fpm_predict(ctx, nullptr, 0, kind, pred.data(), &pred_ms))) {
            std::cerr << "fpm: " << fpm_last_error() << std::endl;
            return 1;
        }
    }
    fpm_info info;
    fpm_get_info_sized(ctx, &info, sizeof info);
    fpm_destroy(ctx);
    fpm_host_close(h);
    bool ok;
    if (!grid) {
        ok = write_npy_c64(out_dir + "/objCrop.npy", objCrop.data(), L, L) &&
             write_npy_c64(out_dir + "/objF.npy", objF.data(), L, L) &&
             write_npy_c64(out_dir + "/pupil.npy", pupil.data(), np, np);
    } else if (blend) {
        ok = write_npy_c64(out_dir + "/objCrop_field.npy", st_field.data(), st_h, st_w) &&
             write_npy_c64_3d(out_dir + "/pupils.npy", pupil.data(), B, np, np);
    } else {
        // stitch: tile b = (i, j) lands at rows i L, columns j L (tiles do not
        // overlap); row-wise copies of L complex values.  With
        // --refocus the tiles placed are the focused ones
        const std::vector<float> &tiles = rf_n > 0 ? rf_focus : objCrop;
        const size_t FW = (size_t)gx * L;
        std::vector<float> field((size_t)gy * L * FW * 2);
        for (int b = 0; b < B; ++b) {
            const int i = b / gx, j = b % gx;
            for (int y = 0; y < L; ++y)
                std::memcpy(&field[(((size_t)i * L + y) * FW + (size_t)j * L) * 2],
                            &tiles[(((size_t)b * L + y) * L) * 2], (size_t)L * 2 * sizeof(float));
        }
        ok = write_npy_c64(out_dir + "/objCrop_field.npy", field.data(), gy * L, gx * L) &&
             write_npy_c64_3d(out_dir + "/pupils.npy", pupil.data(), B, np, np);
    }
    if (ok && write_tiles) ok = write_npy_c64_3d(out_dir + "/objCrop_tiles.npy", objCrop.data(), B, L, L);
    if (ok && !predicted.empty())
        ok = write_npy_4d(out_dir + "/predicted.npy", pred.data(), predicted == "counts" ? "<u2" : "<f4",
                          predicted == "counts" ? 2 : 4, used, B, np, np);
    if (ok && rf_n > 0) ok = write_npy_c64_3d(out_dir + "/objCrop_focus.npy", rf_focus.data(), B, L, L);
    if (ok && write_refocus) ok = write_npy_4d(out_dir + "/refocus.npy", rf_all.data(), "<c8", 8, rf_n, B, L, L);
    if (ok) {  // JSON sidecar describing the arrays (replaces the reference's display windows)
        FILE *f = fopen((out_dir + "/result.json").c_str(), "w");
        ok = f != nullptr;
        if (f) {
            fprintf(f, "{\n  \"dataset\": \"%s\",\n  \"iterations\": %d,\n  \"np\": %d,\n  \"nlarge\": %d,\n",
                    argv[1], itr_count, np, L);
            fprintf(f, "  \"na_radius\": %d,\n  \"delta1\": %g,\n  \"delta2\": %g,\n  \"leds_used\": %d,\n",
                    cfg.na_radius, cfg.delta1, cfg.delta2, used);
            fprintf(f, "  \"device\": %d,\n  \"path\": \"%s\",\n  \"seconds\": %.6f,\n  \"order\": [", device,
                    info.path == FPM_PATH_FUSED ? "fused" : "general", dt);
            for (int i = 0; i < used; ++i) fprintf(f, "%s%d", i ? ", " : "", order[i]);
            fprintf(f, "],\n");
            if (have_pupil0 || have_objf0) {
                // a path as a JSON string (quote, backslash and control characters escaped), or null
                auto quoted = [](const std::string &s) {
                    if (s.empty()) return std::string("null");
                    std::string q = "\"";
                    for (unsigned char ch : s) {
                        char u[8];
                        if (ch == '"' || ch == '\\') q += '\\', q += (char)ch;
                        else if (ch < 0x20) snprintf(u, sizeof u, "\\u%04x", ch), q += u;
                        else q += (char)ch;
                    }
                    return q + "\"";
                };
                fprintf(f, "  \"initial_state\": {\"pupil\": %s, \"pupil_shared\": %s, \"objf\": %s, "
                           "\"replaces_init\": %s},\n",
                        quoted(init_pupil).c_str(), have_pupil0 && pupil0_shared ? "true" : "false",
                        quoted(init_objf).c_str(), have_pupil0 && have_objf0 ? "true" : "false");
            }
            if (want_residual) {
                fprintf(f, "  \"residual\": {\"per_iteration\": [");
                for (size_t i = 0; i < res_iter_e.size(); ++i) put_ratio(f, i ? ", " : "", res_iter_e[i], res_iter_s[i]);
                fprintf(f, "], \"per_patch_last\": [");
                for (int b = 0; b < B; ++b) {
                    double e = 0, s2 = 0;
                    for (int i = 0; i < used; ++i) {
                        e += res_e[(size_t)i * B + b];
                        s2 += res_s[(size_t)i * B + b];
                    }
                    put_ratio(f, b ? ", " : "", e, s2);
                }
                fprintf(f, "], \"per_led_last\": [");
                for (int i = 0; i < used; ++i) {
                    double e = 0, s2 = 0;
                    for (int b = 0; b < B; ++b) {
                        e += res_e[(size_t)i * B + b];
                        s2 += res_s[(size_t)i * B + b];
                    }
                    put_ratio(f, i ? ", " : "", e, s2);
                }
                fprintf(f, "], \"sweep_ms\": %.6f},\n", res_ms);
            }
            if (cal_radius > 0) {  // in processing order (stack index i == position i)
                fprintf(f, "  \"led_calibration\": {\"radius\": %d, \"shift_total\": [", cal_radius);
                for (int i = 0; i < used; ++i)
                    fprintf(f, "%s[%d, %d]", i ? ", " : "", cal_x[i] - x0[i], cal_y[i] - y0[i]);
                fprintf(f, "], \"moved_per_iteration\": [");
                for (size_t i = 0; i < cal_moved.size(); ++i) fprintf(f, "%s%d", i ? ", " : "", cal_moved[i]);
                fprintf(f, "], \"crop_x0\": [");
                for (int i = 0; i < used; ++i) fprintf(f, "%s%d", i ? ", " : "", cal_x[i]);
                fprintf(f, "], \"crop_y0\": [");
                for (int i = 0; i < used; ++i) fprintf(f, "%s%d", i ? ", " : "", cal_y[i]);
                fprintf(f, "], \"probe_ms\": %.6f},\n", cal_ms);
            }
            if (want_gains) {  // in processing order (stack index i == position i)
                fprintf(f, "  \"led_gains\": {\"clip\": [%g, %g], \"gain\": [", gain_lo, gain_hi);
                for (int i = 0; i < used; ++i) {
                    fprintf(f, "%s[", i ? ", " : "");
                    for (int b = 0; b < B; ++b) fprintf(f, "%s%.9g", b ? ", " : "", (double)gain[(size_t)i * B + b]);
                    fprintf(f, "]");
                }
                const std::vector<std::vector<double>> *sums[2] = {&gain_before, &gain_after};
                const char *names[2] = {"before_per_step", "after_per_step"};
                for (int w = 0; w < 2; ++w) {
                    fprintf(f, "], \"%s\": [", names[w]);
                    for (size_t k = 0; k < sums[w]->size(); ++k) {
                        fprintf(f, "%s[", k ? ", " : "");
                        for (int b = 0; b < B; ++b) fprintf(f, "%s%.17g", b ? ", " : "", (*sums[w])[k][b]);
                        fprintf(f, "]");
                    }
                }
                fprintf(f, "], \"moments_ms\": %.6f},\n", gain_ms);
            }
            if (!predicted.empty())
                fprintf(f, "  \"predicted\": {\"kind\": \"%s\", \"shape\": [%d, %d, %d, %d], \"ms\": %.6f},\n",
                        predicted.c_str(), used, B, np, np, pred_ms);
            if (rf_n > 0) {
                auto put_list = [&](const char *name, const std::vector<double> &v) {
                    fprintf(f, "\"%s\": [", name);
                    for (size_t i = 0; i < v.size(); ++i) fprintf(f, "%s%.17g", i ? ", " : "", v[i]);
                    fprintf(f, "], ");
                };
                auto put_table = [&](const char *name, const std::vector<double> &v) {  // [N][patches]
                    fprintf(f, "\"%s\": [", name);
                    for (int k = 0; k < rf_n; ++k) {
                        fprintf(f, "%s[", k ? ", " : "");
                        for (int b = 0; b < B; ++b) fprintf(f, "%s%.17g", b ? ", " : "", v[(size_t)k * B + b]);
                        fprintf(f, "]");
                    }
                    fprintf(f, "], ");
                };
                fprintf(f, "  \"refocus\": {");
                put_list("z", rf_z);
                put_list("zl", rf_zl);
                fprintf(f, "\"fl\": %.17g, \"margin\": %d, \"measure\": \"%s\", \"pick\": \"%s\", ", rf_fl,
                        focus_margin, focus_measure.c_str(), focus_pick.c_str());
                put_table("sum_a", rf_sa);
                put_table("sum_a2", rf_sa2);
                put_table("sum_g", rf_sg);
                fprintf(f, "\"plane\": [");
                for (int b = 0; b < B; ++b) fprintf(f, "%s%d", b ? ", " : "", rf_plane[b]);
                fprintf(f, "], ");
                put_list("z_best", rf_zbest);
                fprintf(f, "\"ms\": %.6f},\n", rf_ms);
            }
            if (blend) {  // factors in row-major patch order, (re, im)
                fprintf(f, "  \"stitch\": {\"overlap\": %d, \"stride\": %d, \"align\": \"%s\", \"field\": [%d, %d], "
                           "\"factors\": [", overlap, st_stride, stitch_align.c_str(), st_h, st_w);
                for (int b = 0; b < B; ++b)
                    fprintf(f, "%s[%.17g, %.17g]", b ? ", " : "", st_factors[2 * b], st_factors[2 * b + 1]);
                fprintf(f, "], \"stitch_ms\": %.6f},\n", st_ms);
            }
            if (grid) {
                fprintf(f, "  \"grid\": {\"gx\": %d, \"gy\": %d, \"patches\": %d, \"frame\": [%d, %d], "
                           "\"patch_origin\": [%d, %d], \"patch_step\": %d},\n  \"bg_val\": [",
                        gx, gy, B, fh, fw, cfg.crop_x, cfg.crop_y, np - std::max(overlap, 0));
                for (int i = 0; i < used; ++i) fprintf(f, "%s%d", i ? ", " : "", bg[i]);
                fprintf(f, "],\n  \"arrays\": {\n");
                if (write_tiles)
                    fprintf(f, "    \"objCrop_tiles.npy\": \"complex64 [gy*gx][Nlarge][Nlarge], IDFT(objF)/Nlarge^2 per "
                               "patch, row-major patch order\",\n");
                if (blend)
                    fprintf(f, "    \"objCrop_field.npy\": \"complex64 [(gy-1)*stride+Nlarge][(gx-1)*stride+Nlarge], "
                               "the patches' objCrop tiles at rows i*stride, columns j*stride times their stitch "
                               "factors, feathered over the overlaps (fpm_stitch)%s\",\n",
                            rf_n > 0 ? "; the tiles are objCrop_focus.npy's, every patch at its plane of best focus" : "");
                else
                    fprintf(f, "    \"objCrop_field.npy\": \"complex64 [gy*Nlarge][gx*Nlarge], patch (i, j) = "
                               "IDFT(objF)/Nlarge^2 of the crop at (cropX + j*Np, cropY + i*Np) at rows i*Nlarge, "
                               "columns j*Nlarge%s\",\n", rf_n > 0 ? ", every patch at its plane of best focus" : "");
                fprintf(f, "    \"pupils.npy\": \"complex64 [gy*gx][Np][Np], centred pupil per patch, row-major "
                           "patch order\"\n  }\n}\n");
            } else {
                fprintf(f, "  \"arrays\": {\n");
                if (write_tiles)
                    fprintf(f, "    \"objCrop_tiles.npy\": \"complex64 [1][Nlarge][Nlarge], objCrop.npy as the one tile of "
                               "a single-patch run\",\n");
                fprintf(f, "    \"objCrop.npy\": \"complex64 [Nlarge][Nlarge], IDFT(objF)/Nlarge^2 (fpmMain.cpp:481)\",\n");
                fprintf(f, "    \"objF.npy\": \"complex64 [Nlarge][Nlarge], un-centred object spectrum\",\n");
                fprintf(f, "    \"pupil.npy\": \"complex64 [Np][Np], centred pupil (fpmMain.cpp:496)\"\n  }\n}\n");
            }
            ok = fclose(f) == 0;
        }
    }
    if (!ok) {
        std::cerr << "cannot write outputs to " << out_dir << std::endl;
        return 1;
    }
    return 0;
}
