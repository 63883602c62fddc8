// tests/cxx/adaptor_keep_frames.cpp -- the reference driver's host sequence (MosaicWithoutPos.cpp:4430-4679) through include/mi355_adaptor.h
// only: SIFT front-end over ImagePoseInfo frames, global alignment, MosaicImagesRefined, MergeImagesRefined.  Built twice by
// tests/test_gpu_adaptor_frames.py: with and without MI355_ADAPTOR_KEEP_FRAMES.
//   adaptor_keep_frames <dir> plain|probe
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), writes <dir>/refined.out and <dir>/merged.out (int32 w, h, then
// the 3 * w bytes of every row).  probe: every frame's pixels are overwritten after extraction -- a render that uploads the caller's
// frames again sees the change, one that reads the kept frames does not.
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
    if (argc < 3) { std::fprintf(stderr, "usage: adaptor_keep_frames <dir> plain|probe\n"); return 2; }
    const std::string dir = argv[1], mode = argv[2];
    if (!mi355::context()) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/images.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open images.bin\n"); return 3; }
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 2 || n > 4096) { std::fclose(f); return 3; }
    std::vector<ImagePoseInfo> poses(n);
    for (int k = 0; k < n; k++) {
        int g[3];
        float h9[9];
        if (std::fread(g, sizeof(int), 3, f) != 3 || g[0] < 16 || g[1] < 16 || g[2] < 3 * g[0]) { std::fclose(f); return 3; }
        IplImage* im = cvCreateImage8U(g[0], g[1], 3);
        if (!im) { std::fclose(f); return 4; }
        std::vector<char> row((size_t)g[2]);
        for (int y = 0; y < g[1]; y++) {                                    // the file's rows are g[2] bytes; the image's are widthStep
            if (std::fread(&row[0], 1, (size_t)g[2], f) != (size_t)g[2]) { std::fclose(f); return 3; }
            std::memcpy(im->imageData + (size_t)y * im->widthStep, &row[0], (size_t)3 * g[0]);
        }
        if (std::fread(h9, sizeof(float), 9, f) != 9) { std::fclose(f); return 3; }
        poses[k].pImg = im;
        poses[k].fixed = k == 0 ? 1 : 0;
    }
    std::fclose(f);
    // :4484-4486 -> GetMatchedPairsOneToAllSIFT_MultiThread
    std::vector<MatchPointPairs> pairs;
    int nSuccess = 0;
    if (mi355::GetMatchedPairsOneToAllSIFT_MultiThread(&poses[0], n, pairs, nSuccess, 2.5f, 3u) != 0) { std::fprintf(stderr, "match: %s\n", mi355_last_error(mi355::context())); return 6; }
    if (mode == "probe")
        for (int k = 0; k < n; k++) std::memset(poses[k].pImg->imageData, 77, (size_t)poses[k].pImg->imageSize);
    // global alignment (:4560-4640), image 0 fixed
    std::vector<ImageTransform> T(n);
    std::vector<int32_t> fixed(n, 0);
    fixed[0] = 1;
    if (mi355_global_affine_align(reinterpret_cast<const mi355_match_point_pairs*>(pairs.empty() ? NULL : &pairs[0]), (int)pairs.size(), n, &fixed[0],
                                  reinterpret_cast<mi355_image_transform*>(&T[0])) != MI355_OK) { std::fprintf(stderr, "align failed\n"); return 7; }
    IplImage* mosaic = NULL;
    if (mi355::MosaicImagesRefined(&poses[0], n, &T[0], mosaic) != 0 || !write_canvas(dir + "/refined.out", mosaic)) { std::fprintf(stderr, "refined failed\n"); return 8; }
    cvReleaseImage(&mosaic);
    if (mi355::MergeImagesRefined(&poses[0], n, &T[0], 1.0f, mosaic) != 0 || !write_canvas(dir + "/merged.out", mosaic)) { std::fprintf(stderr, "merged failed\n"); return 9; }
    cvReleaseImage(&mosaic);
    for (int k = 0; k < n; k++) if (poses[k].pImg) return 10;              // MergeImagesRefined consumed the frames (:2182-2185)
    std::printf("ADAPTOR %s OK pairs %d accepted %d\n", mode.c_str(), (int)pairs.size(), nSuccess);
    return 0;
}
