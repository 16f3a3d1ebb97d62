// vf_predict_steps.hpp -- the IMU steps vf_reserve_node(end) would cut from the IMU buffer at this moment, without consuming them.
// The rule is cut_imu_segment's (vf_graph.cpp; IMUManager::getFactor, IMUManager.cpp:27-74), applied by index to a buffer that
// is only read: samples up to and including `start` are passed over (the last of them is the previous sample; none: a zero
// sample, as in the reference), the samples before `end` give one step each, and if a sample at or beyond `end` follows, one more
// step interpolated at `end`.  Host code, header only (tests/native/predict_steps.cpp checks it on the CPU).
#pragma once

#include <cstddef>
#include <vector>

// Buffer: any indexable sequence (size(), operator[]) of samples with members t, acc[3], gyro[3].  Appends 7 doubles per step
// (dt, acc, gyro) to `steps`.
template <class Buffer>
inline void vf_predict_steps(const Buffer& buffer, double start, double end, std::vector<double>& steps) {
    const size_t n = buffer.size();
    size_t i = 0;
    double pt = 0.0, pa[3] = {0, 0, 0}, pg[3] = {0, 0, 0};
    auto keep = [&](size_t k) {
        pt = buffer[k].t;
        for (int c = 0; c < 3; c++) pa[c] = buffer[k].acc[c], pg[c] = buffer[k].gyro[c];
    };
    while (i < n && buffer[i].t <= start) keep(i++);
    pt = start;
    while (i < n && buffer[i].t < end) {
        const double st[7] = {buffer[i].t - pt, buffer[i].acc[0], buffer[i].acc[1], buffer[i].acc[2], buffer[i].gyro[0], buffer[i].gyro[1], buffer[i].gyro[2]};
        steps.insert(steps.end(), st, st + 7);
        keep(i++);
    }
    if (i < n) {
        const double w = (end - pt) / (buffer[i].t - pt);
        double st[7] = {end - pt, 0, 0, 0, 0, 0, 0};
        for (int c = 0; c < 3; c++) {
            st[1 + c] = w * buffer[i].acc[c] + (1.0 - w) * pa[c];
            st[4 + c] = w * buffer[i].gyro[c] + (1.0 - w) * pg[c];
        }
        steps.insert(steps.end(), st, st + 7);
    }
}
