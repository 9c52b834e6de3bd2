// pinholeStereoCamera.cpp — the dataset-file constructor of PinholeStereoCamera (src/pinholeStereoCamera.cpp:30-125) and the
// rectification of raw stereo pairs (:187-208) over the C-ABI (stvo_rectify_compute on the host, stvo_rectify_* on the GPU).
#include "pinholeStereoCamera.h"

#include <cmath>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>

namespace StVO {

namespace {

// The YAML subset of the dataset parameter files: `key: value` lines, one level of blocks (`cam0:`), scalars and flow lists
// `[a, b, ...]` that may span lines; `#` starts a comment.  Keys of the cam0 block -> their text (lists without the brackets).
std::map<std::string, std::string> read_cam0(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("[PinholeStereoCamera] Invalid parameters file");
    std::map<std::string, std::string> cam;
    std::string raw, block, pending_key, pending;
    bool in_list = false;
    auto trim = [](const std::string& s) {
        const size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r");
        return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
    };
    while (std::getline(f, raw)) {
        std::string line = raw.substr(0, raw.find('#'));
        if (in_list) {
            pending += " " + line;
            if (line.find(']') != std::string::npos) {
                if (block == "cam0") cam[pending_key] = pending;
                in_list = false;
            }
            continue;
        }
        if (trim(line).empty()) continue;
        const bool indented = line[0] == ' ' || line[0] == '\t';
        const size_t colon = line.find(':');
        if (colon == std::string::npos) throw std::runtime_error("[PinholeStereoCamera] cannot read the line: " + raw);
        const std::string key = trim(line.substr(0, colon)), val = trim(line.substr(colon + 1));
        if (!indented) {
            block = val.empty() ? key : std::string();
            continue;
        }
        if (!val.empty() && val[0] == '[' && val.find(']') == std::string::npos) {
            in_list = true;
            pending_key = key;
            pending = val;
            continue;
        }
        if (block == "cam0") cam[key] = val;
    }
    if (in_list) throw std::runtime_error("[PinholeStereoCamera] unterminated list: " + pending_key);
    return cam;
}

const std::string& need(const std::map<std::string, std::string>& cam, const char* key) {
    auto it = cam.find(key);
    if (it == cam.end()) throw std::runtime_error(std::string("[PinholeStereoCamera] missing cam0 key: ") + key);
    return it->second;
}
double scalar(const std::map<std::string, std::string>& cam, const char* key) {
    const std::string& v = need(cam, key);
    char* end = nullptr;
    const double d = std::strtod(v.c_str(), &end);
    if (end == v.c_str()) throw std::runtime_error(std::string("[PinholeStereoCamera] not a number: ") + key);
    return d;
}
std::vector<double> list(const std::map<std::string, std::string>& cam, const char* key) {
    std::string v = need(cam, key);
    const size_t a = v.find('['), b = v.rfind(']');
    if (a == std::string::npos || b == std::string::npos || b < a) throw std::runtime_error(std::string("[PinholeStereoCamera] not a list: ") + key);
    v = v.substr(a + 1, b - a - 1);
    for (char& ch : v)
        if (ch == ',') ch = ' ';
    std::istringstream ss(v);
    ss.imbue(std::locale::classic());
    std::vector<double> out;
    std::string tok;
    while (ss >> tok) out.push_back(std::strtod(tok.c_str(), nullptr));
    return out;
}

}  // namespace

PinholeStereoCamera::PinholeStereoCamera(const std::string& params_file) {
    const auto cam = read_cam0(params_file);
    const auto model = cam.find("cam_model");
    if (model == cam.end() || model->second != "Pinhole") throw std::runtime_error("[PinholeStereoCamera] Invalid cam_model");
    std::memset(&calib, 0, sizeof(calib));
    calib.width = (int)scalar(cam, "cam_width");
    calib.height = (int)scalar(cam, "cam_height");
    calib.b = scalar(cam, "cam_bl");
    if (cam.count("Kl")) {
        calib.form = cam.count("dtype") ? STVO_RECT_FORM_FISHEYE : STVO_RECT_FORM_RADTAN;
        const auto Kl = list(cam, "Kl"), Kr = list(cam, "Kr"), Dl = list(cam, "Dl"), Dr = list(cam, "Dr"), R = list(cam, "R"),
                   t = list(cam, "t");
        if (Kl.size() != 4 || Kr.size() != 4 || Dl.size() != Dr.size() || Dl.size() > 8 || R.size() != 9 || t.size() != 3)
            throw std::runtime_error("[PinholeStereoCamera] Kl / Kr need 4 values, Dl / Dr the same count, R 9 and t 3");
        calib.n_dist = (int)Dl.size();
        for (int i = 0; i < 4; ++i) { calib.Kl[i] = Kl[i]; calib.Kr[i] = Kr[i]; }
        for (int i = 0; i < calib.n_dist; ++i) { calib.Dl[i] = Dl[i]; calib.Dr[i] = Dr[i]; }
        for (int i = 0; i < 9; ++i) calib.R[i] = R[i];
        for (int i = 0; i < 3; ++i) calib.t[i] = t[i];
    } else {
        calib.form = STVO_RECT_FORM_KITTI;
        calib.fx = scalar(cam, "cam_fx"); calib.fy = scalar(cam, "cam_fy");
        calib.cx = scalar(cam, "cam_cx"); calib.cy = scalar(cam, "cam_cy");
        calib.d[0] = scalar(cam, "cam_d0"); calib.d[1] = scalar(cam, "cam_d1");
        calib.d[2] = scalar(cam, "cam_d2"); calib.d[3] = scalar(cam, "cam_d3");
    }
    if (stvo_rectify_compute(&calib, &rect_cam, nullptr, nullptr) != STVO_OK)
        throw std::runtime_error("[PinholeStereoCamera] the calibration cannot be rectified");
    width = rect_cam.width;
    height = rect_cam.height;
    fx = rect_cam.cam.fx; fy = rect_cam.cam.fy; cx = rect_cam.cam.cx; cy = rect_cam.cam.cy; b = rect_cam.cam.b;
    dist = rect_cam.dist != 0;
}

PinholeStereoCamera::~PinholeStereoCamera() {
    if (rectifier) stvo_rectify_destroy(rectifier);
    if (rect_ctx) stvo_ctx_destroy(rect_ctx);
}

void PinholeStereoCamera::ensure_rectifier() const {
    if (rectifier) return;
    if (!rect_ctx && stvo_ctx_create(0, 64, 1, &rect_ctx) != STVO_OK) {
        rect_ctx = nullptr;
        throw std::runtime_error("[PinholeStereoCamera] rectification needs a gfx950 GPU");
    }
    stvo_rectify* r = nullptr;
    int rc;
    if (calib.width > 0) {
        rc = stvo_rectify_create(rect_ctx, 1, &calib, &r);
    } else {  // the parameter constructor: dist = false, the rectifier only copies
        stvo_rect_calib c{};
        c.form = STVO_RECT_FORM_KITTI;
        c.width = width; c.height = height;
        c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.b = b;
        rc = stvo_rectify_create(rect_ctx, 1, &c, &r);
    }
    if (rc != STVO_OK) throw std::runtime_error(std::string("[PinholeStereoCamera] stvo_rectify_create: ") + stvo_error_string(rc));
    rectifier = r;
}

void PinholeStereoCamera::rectifyImagesLR(const GrayImage& src_l, std::vector<uint8_t>& dst_l, const GrayImage& src_r,
                                          std::vector<uint8_t>& dst_r) const {
    if (src_l.rows != height || src_l.cols != width || src_r.rows != height || src_r.cols != width || src_l.empty() || src_r.empty())
        throw std::invalid_argument("[PinholeStereoCamera] rectifyImagesLR: images must be width x height");
    ensure_rectifier();
    const size_t px = (size_t)width * height;
    // contiguous copies of the sources: covers strided views and in-place calls (dst aliasing src) alike
    std::vector<uint8_t> in(2 * px), out(2 * px);
    for (int s = 0; s < 2; ++s) {
        const GrayImage& g = s ? src_r : src_l;
        const size_t step = g.step ? g.step : (size_t)g.cols;
        for (int y = 0; y < height; ++y) std::memcpy(in.data() + s * px + (size_t)y * width, g.data + y * step, (size_t)width);
    }
    const int rc = stvo_rectify_images(rectifier, 1, in.data(), in.data() + px, out.data(), out.data() + px);
    if (rc != STVO_OK) throw std::runtime_error(std::string("[PinholeStereoCamera] stvo_rectify_images: ") + stvo_error_string(rc));
    dst_l.assign(out.begin(), out.begin() + px);
    dst_r.assign(out.begin() + px, out.end());
}

void PinholeStereoCamera::rectifyImage(const GrayImage& img_src, std::vector<uint8_t>& img_rec) const {
    // the reference remaps with the left map (:189-192)
    std::vector<uint8_t> unused;
    rectifyImagesLR(img_src, img_rec, img_src, unused);
}

// Colour images: cv::remap works on every channel of the Mat, each rounded to 8 bits on its own (stvo_rectify_color_images).
void PinholeStereoCamera::rectifyImagesLR(const Image& src_l, std::vector<uint8_t>& dst_l, const Image& src_r, std::vector<uint8_t>& dst_r) const {
    if (src_l.channels == 1 && src_r.channels == 1) return rectifyImagesLR(src_l.gray(), dst_l, src_r.gray(), dst_r);
    const int ch = src_l.channels;
    if (src_l.rows != height || src_l.cols != width || src_r.rows != height || src_r.cols != width || src_l.empty() || src_r.empty() ||
        src_r.channels != ch || (ch != 3 && ch != 4))
        throw std::invalid_argument("[PinholeStereoCamera] rectifyImagesLR: images must be width x height with 1, 3 or 4 channels, both alike");
    ensure_rectifier();
    const size_t row = (size_t)width * ch, bytes = row * height;
    std::vector<uint8_t> in(2 * bytes), out(2 * bytes);  // contiguous copies, as above
    for (int s = 0; s < 2; ++s) {
        const Image& g = s ? src_r : src_l;
        const size_t step = g.step ? g.step : row;
        for (int y = 0; y < height; ++y) std::memcpy(in.data() + s * bytes + (size_t)y * row, g.data + y * step, row);
    }
    const int rc = stvo_rectify_color_images(rectifier, 1, ch, in.data(), in.data() + bytes, out.data(), out.data() + bytes);
    if (rc != STVO_OK) throw std::runtime_error(std::string("[PinholeStereoCamera] stvo_rectify_color_images: ") + stvo_error_string(rc));
    dst_l.assign(out.begin(), out.begin() + bytes);
    dst_r.assign(out.begin() + bytes, out.end());
}

void PinholeStereoCamera::rectifyImage(const Image& img_src, std::vector<uint8_t>& img_rec) const {
    std::vector<uint8_t> unused;
    rectifyImagesLR(img_src, img_rec, img_src, unused);
}

}  // namespace StVO
