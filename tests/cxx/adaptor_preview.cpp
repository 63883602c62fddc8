// tests/cxx/adaptor_preview.cpp -- mi355::MosaicImagesPreview through include/mi355_adaptor.h alone, on frames and transforms read from a file.
// Built and run by tests/test_gpu_adaptor_preview.py, which compares the images with those of the C ABI call.
//   adaptor_preview <dir>
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), writes <dir>/preview_r<render>_l<level>.out for render 0, 1, 2 at
// level 2 and for render 2 at level 5 (int32 w, h, then the 3 * w bytes of every row).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mi355_adaptor.h"

using namespace mi355ref;

static bool write_canvas(const std::string& path, const IplImage* im) {
    if (!im) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const int wh[2] = {im->width, im->height};
    std::fwrite(wh, sizeof(int), 2, f);
    for (int y = 0; y < im->height; y++) std::fwrite(im->imageData + (size_t)y * im->widthStep, 1, (size_t)3 * im->width, f);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_preview <dir>\n"); return 2; }
    const std::string dir = argv[1];
    if (!mi355::context()) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/images.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open images.bin\n"); return 3; }
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 2 || n > 4096) { std::fclose(f); return 3; }
    std::vector<ImagePoseInfo> poses(n);
    std::vector<ImageTransform> T(n);
    for (int k = 0; k < n; k++) {
        int g[3];
        if (std::fread(g, sizeof(int), 3, f) != 3 || g[0] < 2 || g[1] < 2 || g[2] < 3 * g[0]) { std::fclose(f); return 3; }
        IplImage* im = cvCreateImage8U(g[0], g[1], 3);
        if (!im) { std::fclose(f); return 4; }
        std::vector<char> row((size_t)g[2]);
        for (int y = 0; y < g[1]; y++) {                                    // the file's rows are g[2] bytes; the image's are widthStep
            if (std::fread(&row[0], 1, (size_t)g[2], f) != (size_t)g[2]) { std::fclose(f); return 3; }
            std::memcpy(im->imageData + (size_t)y * im->widthStep, &row[0], (size_t)3 * g[0]);
        }
        if (std::fread(T[k].h.m, sizeof(float), 9, f) != 9) { std::fclose(f); return 3; }
        poses[k].pImg = im;
        poses[k].fixed = k == 0 ? 1 : 0;
    }
    std::fclose(f);
    IplImage* mosaic = NULL;
    const int jobs[4][2] = {{0, 2}, {1, 2}, {2, 2}, {2, 5}};                 // render, level; every call releases and replaces the last image
    for (int j = 0; j < 4; j++) {
        char name[64];
        std::snprintf(name, sizeof(name), "/preview_r%d_l%d.out", jobs[j][0], jobs[j][1]);
        if (mi355::MosaicImagesPreview(&poses[0], n, &T[0], jobs[j][1], jobs[j][0], mosaic) != 0 || !write_canvas(dir + name, mosaic)) {
            std::fprintf(stderr, "preview render %d level %d failed: %s\n", jobs[j][0], jobs[j][1], mi355_last_error(mi355::context()));
            return 8;
        }
    }
    // argument refusals: MosaicImagesSeamline's, and a level or a render outside its range; the image is left as it is
    IplImage* before = mosaic;
    if (mi355::MosaicImagesPreview((const ImagePoseInfo*)NULL, n, &T[0], 3, 0, mosaic) != -1) return 11;
    if (mi355::MosaicImagesPreview(&poses[0], 1, &T[0], 3, 0, mosaic) != -2) return 12;
    if (mi355::MosaicImagesPreview(&poses[0], n, &T[0], 0, 0, mosaic) != -1 || mi355::MosaicImagesPreview(&poses[0], n, &T[0], 8, 0, mosaic) != -1) return 13;
    if (mi355::MosaicImagesPreview(&poses[0], n, &T[0], 3, 3, mosaic) != -1 || mosaic != before) return 14;
    // and the adaptor goes on working
    if (mi355::MosaicImagesPreview(&poses[0], n, &T[0], 2, 2, mosaic) != 0 || !write_canvas(dir + "/preview_again.out", mosaic)) return 15;
    cvReleaseImage(&mosaic);
    for (int k = 0; k < n; k++) cvReleaseImage(&poses[k].pImg);
    std::printf("ADAPTOR PREVIEW OK frames %d\n", n);
    return 0;
}
