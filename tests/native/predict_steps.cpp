// tests/native/predict_steps.cpp -- vf_predict_steps (vil_sensor_fusion_amd/csrc/vf_predict_steps.hpp) on the CPU: a hand-written
// timeline, the same steps as cut_imu_segment's rule for a cut at `time` (restated here on a copy that it consumes, as
// vf_graph.cpp does), and the buffer left as it was -- including the reference's zero previous sample when nothing precedes the start.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "vf_graph_handle.hpp"
#include "vf_predict_steps.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static ImuSample sample(double t, double a, double g) { return ImuSample{t, {a, 2 * a, 3 * a}, {g, -g, 0.5 * g}}; }

// cut_imu_segment's rule as vf_graph.cpp states it (IMUManager.cpp:27-74), consuming the buffer it is given
static void cut_consuming(std::deque<ImuSample>& buffer, double start, double end, std::vector<double>& steps) {
    ImuSample prev{};
    while (!buffer.empty() && buffer.front().t <= start) { prev = buffer.front(); buffer.pop_front(); }
    prev.t = start;
    while (!buffer.empty() && buffer.front().t < end) {
        const ImuSample m = buffer.front();
        buffer.pop_front();
        const double st[7] = {m.t - prev.t, m.acc[0], m.acc[1], m.acc[2], m.gyro[0], m.gyro[1], m.gyro[2]};
        steps.insert(steps.end(), st, st + 7);
        prev = m;
    }
    if (!buffer.empty()) {
        const ImuSample& f = buffer.front();
        const double w = (end - prev.t) / (f.t - prev.t);
        double st[7] = {end - prev.t, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 3; i++) {
            st[1 + i] = w * f.acc[i] + (1.0 - w) * prev.acc[i];
            st[4 + i] = w * f.gyro[i] + (1.0 - w) * prev.gyro[i];
        }
        steps.insert(steps.end(), st, st + 7);
    }
}

static bool same_buffer(const std::deque<ImuSample>& a, const std::deque<ImuSample>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (memcmp(&a[i], &b[i], sizeof(ImuSample)) != 0) return false;
    return true;
}

static void against_the_rule(const std::deque<ImuSample>& buffer, double start, double end) {
    const std::deque<ImuSample> before = buffer;
    std::vector<double> got, want;
    vf_predict_steps(buffer, start, end, got);
    CHECK(same_buffer(buffer, before));                   // nothing consumed, nothing changed
    std::deque<ImuSample> copy = buffer;
    cut_consuming(copy, start, end, want);
    CHECK(got.size() == want.size());
    CHECK(got.size() == want.size() && (got.empty() || memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0));   // bit for bit
}

int main() {
    // samples at 0.00, 0.01, .. 0.09
    std::deque<ImuSample> buf;
    for (int i = 0; i < 10; i++) buf.push_back(sample(0.01 * i, 1.0 + i, 0.1 * i));

    {   // hand-written timeline: cut (0.025, 0.052]: previous sample 0.02; steps at 0.03, 0.04, 0.05; interpolated at 0.052 towards 0.06
        std::vector<double> s;
        vf_predict_steps(buf, 0.025, 0.052, s);
        CHECK(s.size() == 4 * 7);
        if (s.size() == 28) {
            CHECK(std::fabs(s[0] - 0.005) < 1e-15 && s[1] == 4.0 && s[2] == 8.0 && s[3] == 12.0 && s[4] == 0.1 * 3);
            CHECK(std::fabs(s[7] - 0.01) < 1e-15 && s[8] == 5.0);
            CHECK(std::fabs(s[14] - 0.01) < 1e-15 && s[15] == 6.0);
            const double w = (0.052 - 0.05) / (0.06 - 0.05);
            CHECK(std::fabs(s[21] - 0.002) < 1e-15);
            CHECK(s[22] == w * 7.0 + (1.0 - w) * 6.0 && s[25] == w * (0.1 * 6) + (1.0 - w) * (0.1 * 5));
            double total = 0;
            for (int i = 0; i < 4; i++) total += s[7 * i];
            CHECK(std::fabs(total - (0.052 - 0.025)) < 1e-15);
        }
    }
    {   // a cut that ends exactly at a sample: that sample is the interpolated step, with weight one
        std::vector<double> s;
        vf_predict_steps(buf, 0.02, 0.04, s);
        CHECK(s.size() == 2 * 7);
        if (s.size() == 14) CHECK(s[8] == 5.0 && s[11] == 0.1 * 4 && std::fabs(s[7] - 0.01) < 1e-15);
    }
    {   // beyond the last sample: every remaining sample, no interpolated step
        std::vector<double> s;
        vf_predict_steps(buf, 0.065, 1.0, s);
        CHECK(s.size() == 3 * 7);
    }
    {   // nothing precedes the start: the reference's quirk, a ZERO previous sample enters the interpolation
        std::vector<double> s;
        vf_predict_steps(buf, -1.0, -0.5, s);
        CHECK(s.size() == 7);
        if (s.size() == 7) {
            const double w = (-0.5 - -1.0) / (0.0 - -1.0);
            CHECK(s[0] == 0.5 && s[1] == w * 1.0 + (1.0 - w) * 0.0 && s[4] == 0.0);
        }
    }
    {   // an empty buffer gives nothing; appending to steps that are there already keeps them
        std::deque<ImuSample> none;
        std::vector<double> s(7, 42.0);
        vf_predict_steps(none, 0.0, 1.0, s);
        CHECK(s.size() == 7 && s[0] == 42.0);
        vf_predict_steps(buf, 0.0, 0.015, s);
        CHECK(s.size() == 3 * 7 && s[6] == 42.0);
    }
    // the same steps as the consuming rule, the buffer untouched: cuts inside, at samples, before, beyond, of zero length
    const double cuts[][2] = {{0.025, 0.052}, {0.02, 0.04}, {0.0, 0.09}, {0.065, 1.0}, {-1.0, -0.5}, {-1.0, 0.0}, {0.03, 0.03}, {0.031, 0.031},
                              {0.09, 0.2}, {0.5, 0.6}, {0.0, 0.001}};
    for (const auto& c : cuts) against_the_rule(buf, c[0], c[1]);
    {   // two samples that share a timestamp (a zero-dt step)
        std::deque<ImuSample> dup = buf;
        dup.insert(dup.begin() + 4, sample(0.03, 9.0, 9.0));
        against_the_rule(dup, 0.01, 0.055);
        against_the_rule(dup, 0.03, 0.055);
    }
    {   // a std::vector is a buffer too (by index, no deque needed)
        std::vector<ImuSample> vec(buf.begin(), buf.end());
        std::vector<double> a, b;
        vf_predict_steps(vec, 0.025, 0.052, a);
        vf_predict_steps(buf, 0.025, 0.052, b);
        CHECK(a == b);
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("predict_steps ok\n");
    return 0;
}
