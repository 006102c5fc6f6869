// fovpt_camera.h -- the inverse of a camera's [U V W], host code: what fovpt_temporal, fovpt_warp, fovpt_lens and the depth
// packet (api_post.hip, api_view.hip, api_packet.hip) and the depth packet's checks for a client (packet_host.cpp, also in
// libfovpt_loader.so) all compute, in one place.
#pragma once
#include <cmath>

// The rows of [U V W]^-1 (U, V, W the columns), in binary64: det = U . (V x W), rows (V x W) / det, (W x U) / det,
// (U x V) / det, each entry rounded to binary32.  false: det is 0 or not finite.
inline bool fovpt_camera_inverse(const float* U, const float* V, const float* W, float* inv)
{
    auto cross = [](const double* a, const double* b, double* r) {
        r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
    };
    const double u[3] = {U[0], U[1], U[2]}, v[3] = {V[0], V[1], V[2]}, w[3] = {W[0], W[1], W[2]};
    double r[3][3];
    cross(v, w, r[0]); cross(w, u, r[1]); cross(u, v, r[2]);
    const double det = (u[0] * r[0][0] + u[1] * r[0][1]) + u[2] * r[0][2];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) inv[3 * i + j] = (float)(r[i][j] / det);
    return true;
}
