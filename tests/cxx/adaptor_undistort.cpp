// tests/cxx/adaptor_undistort.cpp -- lens undistortion through include/mi355_adaptor.h alone, on a frame, a camera and parameters read from
// a file: mi355::UndistortImage into a second IplImage, with and without parameters, and in place.  Built and run by
// tests/test_gpu_adaptor_undistort.py, which compares the images with those of the C ABI call.
//   adaptor_undistort <dir>
// reads <dir>/frame.bin (int32 w, h, fill, pad; 9 doubles of the camera; out_fx, out_fy, out_cx, out_cy; then the 3 * w bytes of every row),
// writes <dir>/fitted.out, <dir>/own.out and <dir>/inplace.out (int32 w, h, then int64 n_outside, then the 3 * w bytes of every row).
#include <cstdio>
#include <cstring>
#include <string>
#include "mi355_adaptor.h"

using namespace mi355ref;

static bool write_image(const std::string& path, const IplImage* im, long long n_outside) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const int wh[2] = {im->width, im->height};
    std::fwrite(wh, sizeof(int), 2, f);
    std::fwrite(&n_outside, sizeof(long long), 1, f);
    for (int y = 0; y < im->height; y++) std::fwrite(im->imageData + (size_t)y * im->widthStep, 1, (size_t)3 * im->width, f);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_undistort <dir>\n"); return 2; }
    const std::string dir = argv[1];
    if (!mi355::context()) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/frame.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open frame.bin\n"); return 3; }
    int g[4];
    mi355_camera cam;
    mi355_undistort_params prm;
    mi355_default_undistort_params(&prm);
    if (std::fread(g, sizeof(int), 4, f) != 4 || g[0] < 2 || g[1] < 2 || std::fread(&cam, sizeof(double), 9, f) != 9 ||
        std::fread(&prm.out_fx, sizeof(double), 4, f) != 4) { std::fclose(f); return 3; }
    prm.fill = g[2];
    IplImage* src = cvCreateImage8U(g[0], g[1], 3);
    IplImage* dst = cvCreateImage8U(g[0], g[1], 3);
    if (!src || !dst) { std::fclose(f); return 4; }
    std::memset(dst->imageData, 0x5a, (size_t)dst->imageSize);
    for (int y = 0; y < g[1]; y++)
        if (std::fread(src->imageData + (size_t)y * src->widthStep, 1, (size_t)3 * g[0], f) != (size_t)3 * g[0]) { std::fclose(f); return 3; }
    std::fclose(f);
    long long n_out = -1;
    if (mi355::UndistortImage(src, dst, cam, &prm, &n_out) != 0 || !write_image(dir + "/fitted.out", dst, n_out)) { std::fprintf(stderr, "fitted failed: %s\n", mi355_last_error(mi355::context())); return 8; }
    // the row padding of the destination is not written
    for (int y = 0; y < g[1]; y++)
        for (int b = 3 * g[0]; b < dst->widthStep; b++)
            if ((unsigned char)dst->imageData[(size_t)y * dst->widthStep + b] != 0x5a) return 9;
    if (mi355::UndistortImage(src, dst, cam) != 0 || !write_image(dir + "/own.out", dst, 0)) return 10;                 // no parameters: the camera's own intrinsics, fill 0
    if (mi355::UndistortImage(src, src, cam, &prm, &n_out) != 0 || !write_image(dir + "/inplace.out", src, n_out)) return 11;
    // argument refusals
    IplImage* small = cvCreateImage8U(g[0] - 1, g[1], 3);
    IplImage* gray = cvCreateImage8U(g[0], g[1], 1);
    if (mi355::UndistortImage((const IplImage*)NULL, dst, cam) != -1 || mi355::UndistortImage(src, (IplImage*)NULL, cam) != -1) return 12;
    if (mi355::UndistortImage(src, small, cam) != -1 || mi355::UndistortImage(gray, gray, cam) != -1) return 13;
    prm.fill = 300;
    if (mi355::UndistortImage(src, dst, cam, &prm) != MI355_ERR_ARG) return 14;
    cvReleaseImage(&small); cvReleaseImage(&gray); cvReleaseImage(&src); cvReleaseImage(&dst);
    std::printf("ADAPTOR UNDISTORT OK %d x %d\n", g[0], g[1]);
    return 0;
}
