// view_change_plugin.cpp — NFGPUKernelModule::AddObjectEnterCallBack / AddObjectLeaveCallBack
// (include/NFGPUKernelModule.hpp) from a game-server-style client: the script of
// tests/view_change_model.py (the golden script of tests/golden/view_change.json: SCENE / GRP / OBJ lines,
// INIT, then windows of SW / CR / DE closed by X) is replayed through the plugin API on a GPU world.
// Every window's Execute() delivers the window's enter / leave calls; each prints, in the format of
// tests/cpp/view_change_ref.cpp,
//   E|L <to, script indices> : <about, script indices>
// which tests/test_gpu_view_change.py compares with the recorded calls of the compiled reference.
// (GRP makes a group exist in the reference; a world has no such call: a group is its members.)
//
// usage: view_change_plugin <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "NFGPUKernelModule.hpp"

using namespace nfgpu;

static int64_t g_now = 1000;
static std::map<NFGUID, int> g_index;

static NFGUID guid_of(int i) { return NFGUID(7, (i * 37) % 101 + 1); }  // tests.view_change_model.script_guid

static int print_call(const char* k, const std::vector<NFGUID>& to, const std::vector<NFGUID>& about) {
    printf("%s", k);
    for (const NFGUID& g : to) printf(" %d", g_index.at(g));
    printf(" :");
    for (const NFGUID& g : about) printf(" %d", g_index.at(g));
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    NFGPUKernelModule km(256);
    km.SetTimeSource([] { return g_now; });
    km.AddProperty("SceneID", TDATA_INT);
    km.AddProperty("GroupID", TDATA_INT);
    km.AddProperty("X", TDATA_FLOAT);
    km.AddProperty("Y", TDATA_FLOAT);
    km.AddProperty("Z", TDATA_FLOAT);
    km.AddClass("NPC");
    km.AddClass("Player");
    for (const char* c : {"NPC", "Player"})
        for (const char* p : {"SceneID", "GroupID", "X", "Y", "Z"}) km.SetPropertyFlags(c, p, true, true, false);
    km.Init();
    km.AddObjectEnterCallBack([](const std::vector<NFGUID>& to, const std::vector<NFGUID>& about) {
        return print_call("E", to, about);
    });
    km.AddObjectLeaveCallBack([](const std::vector<NFGUID>& to, const std::vector<NFGUID>& about) {
        return print_call("L", to, about);
    });
    auto create = [&](int i, const std::string& cls, int s, int g) {
        g_index[guid_of(i)] = i;
        return km.CreateObject(guid_of(i), s, g, cls == "P" ? "Player" : "NPC", {});
    };
    std::string ln;
    while (std::getline(in, ln)) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (f.empty()) continue;
        const std::string& op = f[0];
        auto I = [&](size_t k) { return atoi(f[k].c_str()); };
        if (op == "SCENE") {
            if (!km.CreateScene(I(1))) return 3;
        } else if (op == "GRP") {
        } else if (op == "OBJ" || op == "CR") {
            if (!create(I(1), f[2], I(3), I(4))) return 4;
        } else if (op == "INIT") {
            km.AfterInit();
            g_now += 100;
            km.Execute();  // (objects created before AfterInit are no calls of a window: nothing is delivered)
        } else if (op == "SW") {
            if (!km.SwitchScene(guid_of(I(1)), I(2), I(3), 1.0f, 2.0f, 3.0f)) return 5;
        } else if (op == "DE") {
            if (!km.DestroyObject(guid_of(I(1)))) return 6;
        } else if (op == "X") {
            g_now += 100;
            km.Execute();
        } else {
            return 7;
        }
    }
    km.BeforeShut();
    km.Shut();
    return 0;
}
