// pinholeStereoCamera.h — the camera scalars and the two functions the path uses (src/pinholeStereoCamera.cpp:221-237,
// include/pinholeStereoCamera.h:75-90), and the dataset-file constructor with its rectification (:30-125, :196-208).
//   - PinholeStereoCamera(width, height, fx, fy, cx, cy, b): parameters given directly, images assumed rectified (dist = false).
//   - PinholeStereoCamera(params_file): reads the dataset parameter file (a `cam0:` block of scalars and flow lists, the subset
//     config/dataset_params/*.yaml use) and takes the reference's branch: KITTI-style undistortion (cam_d0 != 0), stereoRectify +
//     initUndistortRectifyMap (Kl, Kr, Dl, Dr, R, t) or the fisheye maps (a `dtype` key).  The rectification maths run on the host
//     (stvo_rectify_compute); fx, fy, cx, cy come from P1 and b is cam_bl.  Throws std::runtime_error on a file it cannot read.
//   - rectifyImage / rectifyImagesLR: cv::remap(INTER_LINEAR) with those maps, bit for bit, on the GPU (stvo_rectify_*), or a copy
//     when dist is false.  The GPU rectifier is created on the first call, so constructing a camera needs no GPU; the call
//     throws std::runtime_error when no device is available.  In-place use (dst aliasing src, as the reference's
//     Dataset::nextFrame calls it) goes through a temporary.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/stvo_hip.h"
#include "stvo_compat.h"

namespace StVO {

class PinholeStereoCamera {
public:
    PinholeStereoCamera(int width_, int height_, double fx_, double fy_, double cx_, double cy_, double b_)
        : width(width_), height(height_), fx(fx_), fy(fy_), cx(cx_), cy(cy_), b(b_) {}
    explicit PinholeStereoCamera(const std::string& params_file);
    ~PinholeStereoCamera();
    PinholeStereoCamera(const PinholeStereoCamera&) = delete;
    PinholeStereoCamera& operator=(const PinholeStereoCamera&) = delete;

    int getWidth() const { return width; }
    int getHeight() const { return height; }
    double getB() const { return b; }
    double getFx() const { return fx; }
    double getFy() const { return fy; }
    double getCx() const { return cx; }
    double getCy() const { return cy; }
    bool getDist() const { return dist; }
    // R1 / R2 / P1 / P2 of the rectification (identity / zero for the parameter constructor)
    const stvo_rect_camera& getRectification() const { return rect_cam; }
    Vector3d backProjection(const double& u, const double& v, const double& disp) const {
        Vector3d P;
        const double bd = b / disp;
        P(0) = bd * (u - cx);
        P(1) = bd * (v - cy);
        P(2) = bd * fx;
        return P;
    }
    Vector2d projection(const Vector3d& P) const {
        Vector2d uv;
        uv(0) = cx + fx * P(0) / P(2);
        uv(1) = cy + fy * P(1) / P(2);
        return uv;
    }
    stvo_cam abi() const { return stvo_cam{fx, fy, cx, cy, b}; }

    // src/pinholeStereoCamera.cpp:187-208.  Images are width x height bytes; dst is resized to width * height.
    void rectifyImage(const GrayImage& img_src, std::vector<uint8_t>& img_rec) const;
    void rectifyImagesLR(const GrayImage& img_src_l, std::vector<uint8_t>& img_rec_l, const GrayImage& img_src_r,
                         std::vector<uint8_t>& img_rec_r) const;
    // The same on colour images (3 or 4 interleaved channels, every channel remapped; one channel forwards to the overloads above):
    // dst is resized to width * height * channels.
    void rectifyImage(const Image& img_src, std::vector<uint8_t>& img_rec) const;
    void rectifyImagesLR(const Image& img_src_l, std::vector<uint8_t>& img_rec_l, const Image& img_src_r, std::vector<uint8_t>& img_rec_r) const;

private:
    void ensure_rectifier() const;

    int width, height;
    double fx, fy, cx, cy, b;
    bool dist = false;
    stvo_rect_calib calib{};
    stvo_rect_camera rect_cam{};
    mutable stvo_ctx* rect_ctx = nullptr;
    mutable stvo_rectify* rectifier = nullptr;
};

}  // namespace StVO
