// tests/cxx/adaptor_median.cpp -- the median render through include/mi355_adaptor.h alone, on frames and transforms read from a file:
// MosaicImagesMedian, and MosaicImagesSeamline after it into the same result pointer.  Built and run by tests/test_gpu_adaptor_median.py, which
// compares the canvases with those of the C ABI calls.
//   adaptor_median <dir>
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), writes <dir>/median.out and <dir>/seamline.out (int32 w, h,
// then the 3 * w bytes of every row).
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
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_median <dir>\n"); return 2; }
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
    if (mi355::MosaicImagesMedian(&poses[0], n, &T[0], mosaic) != 0 || !write_canvas(dir + "/median.out", mosaic)) { std::fprintf(stderr, "median failed: %s\n", mi355_last_error(mi355::context())); return 8; }
    // a second call releases the first canvas and replaces it, like the other wrappers
    if (mi355::MosaicImagesSeamline(&poses[0], n, &T[0], mosaic) != 0 || !write_canvas(dir + "/seamline.out", mosaic)) { std::fprintf(stderr, "seamline failed\n"); return 9; }
    cvReleaseImage(&mosaic);
    // argument refusals, as MosaicImagesSeamline's
    if (mi355::MosaicImagesMedian((const ImagePoseInfo*)NULL, n, &T[0], mosaic) != -1) return 11;
    if (mi355::MosaicImagesMedian(&poses[0], 1, &T[0], mosaic) != -2 || mosaic) return 12;
    for (int k = 0; k < n; k++) cvReleaseImage(&poses[k].pImg);
    std::printf("ADAPTOR MEDIAN OK frames %d\n", n);
    return 0;
}
