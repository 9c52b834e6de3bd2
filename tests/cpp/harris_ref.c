/* A plain-C statement of OpenCV's HarrisResponses (features2d/src/orb.cpp; blockSize 7, harris_k 0.04f) for one key-point: test
 * infrastructure, the second statement beside tests/np_harris.py.  Built with -ffp-contract=off: every float operation rounds once. */
#include <stdint.h>

float harris_response_sums(int a, int b, int c) {
    const float harris_k = 0.04f;
    float scale = 1.f / ((1 << 2) * 7 * 255.f);
    float scale_sq_sq = scale * scale * scale * scale;
    return ((float)a * b - (float)c * c - harris_k * ((float)a + b) * ((float)a + b)) * scale_sq_sq;
}

/* img: 8-bit, `step` bytes per row; (x, y): the key-point, at least 4 pixels from every border */
float harris_response(const uint8_t* img, int step, int x, int y, int* abc) {
    const int r = 7 / 2;
    const uint8_t* ptr0 = img + (y - r) * step + (x - r);
    int a = 0, b = 0, c = 0;
    for (int k = 0; k < 49; ++k) {
        const uint8_t* ptr = ptr0 + (k / 7) * step + (k % 7);
        int Ix = (ptr[1] - ptr[-1]) * 2 + (ptr[-step + 1] - ptr[-step - 1]) + (ptr[step + 1] - ptr[step - 1]);
        int Iy = (ptr[step] - ptr[-step]) * 2 + (ptr[step - 1] - ptr[-step - 1]) + (ptr[step + 1] - ptr[-step + 1]);
        a += Ix * Ix;
        b += Iy * Iy;
        c += Ix * Iy;
    }
    if (abc) {
        abc[0] = a;
        abc[1] = b;
        abc[2] = c;
    }
    return harris_response_sums(a, b, c);
}

void harris_responses(const uint8_t* img, int cols, int n, const int32_t* xs, const int32_t* ys, float* out, int32_t* abc) {
    for (int i = 0; i < n; ++i) out[i] = harris_response(img, cols, xs[i], ys[i], abc ? abc + 3 * i : 0);
}
