// view_change_ref.cpp — the reference's own OnObjectListEnter / OnObjectListLeave calls, for
// tests/golden/view_change.json.  The script of tests/view_change_model.py (golden_script(): SCENE / GRP /
// OBJ lines, INIT, then windows of SW / CR / DE closed by X) is replayed on the reference's
// NFCKernelModule + NFCSceneAOIModule (compiled from the reference tree where it lies; see
// tests/golden/gen_view_change_golden.py) with the AOI module's common callbacks LEFT REGISTERED: its
// OnGroupEvent / OnSceneEvent / OnClassCommonEvent (AOI:292-529) run inside every SwitchScene,
// CreateObject and DestroyObject.  ReleaseGroupScene (called on every group leave, AOI:389-393) is
// overridden to record the call and do nothing.  From INIT on every enter / leave callback prints
//   E|L <to, script indices> : <about, script indices>
// (the format of tests/cpp/view_change_plugin.cpp) and every neutralised release "R <scene> <group>".
// The reference applies a call at once, so the frame line "X" does nothing here.  TEST INFRASTRUCTURE,
// run by hand on a machine that has the reference tree.
//
// usage: view_change_ref <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include "NFComm/NFKernelPlugin/NFCEventModule.h"
#include "NFComm/NFKernelPlugin/NFCKernelModule.h"
#include "NFComm/NFKernelPlugin/NFCScheduleModule.h"
#include "NFComm/NFKernelPlugin/NFCSceneAOIModule.h"
#include "NFComm/NFConfigPlugin/NFCClassModule.h"
#include "NFComm/NFConfigPlugin/NFCElementModule.h"
#include "../../oracle/nfio.h"
#include "../../oracle/ref_server.hpp"

extern "C" int clock_gettime(clockid_t clk, struct timespec* ts) {  // NFGetTime(): the session clock
    if (clk == CLOCK_REALTIME) {
        ts->tv_sec = g_now / 1000;
        ts->tv_nsec = (g_now % 1000) * 1000000;
        return 0;
    }
    return (int)syscall(SYS_clock_gettime, clk, ts);
}

static bool g_print = false;
static std::map<NFGUID, int> g_index;

struct ViewKernel : NFCKernelModule {
    using NFCKernelModule::NFCKernelModule;
    bool ReleaseGroupScene(const int nSceneID, const int nGroupID) override {
        if (g_print) printf("R %d %d\n", nSceneID, nGroupID);
        return false;
    }
};

struct Printer {
    int line(const char* k, const NFIDataList& to, const NFIDataList& about) {
        if (!g_print) return 0;
        printf("%s", k);
        for (int i = 0; i < to.GetCount(); i++) printf(" %d", g_index.at(to.Object(i)));
        printf(" :");
        for (int i = 0; i < about.GetCount(); i++) printf(" %d", g_index.at(about.Object(i)));
        printf("\n");
        return 0;
    }
    int OnEnter(const NFIDataList& to, const NFIDataList& about) { return line("E", to, about); }
    int OnLeave(const NFIDataList& to, const NFIDataList& about) { return line("L", to, about); }
};

static NFGUID guid_of(int i) { return NFGUID(7, (i * 37) % 101 + 1); }  // tests.view_change_model.script_guid

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;

    TestPluginManager pm;
    auto prop = [](const char* id, const char* type) {
        return std::string("<Property Id=\"") + id + "\" Type=\"" + type +
               "\" Public=\"1\" Private=\"1\" Save=\"0\" Cache=\"0\" Ref=\"0\" Upload=\"0\"/>";
    };
    pm.files["NFDataCfg/Struct/LogicClass.xml"] =
        "<XML><Class Id=\"IObject\" Type=\"TYPE_IOBJECT\" Path=\"NFDataCfg/Struct/Class/IObject.xml\" InstancePath=\"\">"
        "<Class Id=\"NPC\" Type=\"TYPE_NPC\" Path=\"NFDataCfg/Struct/Class/NPC.xml\" InstancePath=\"\"/>"
        "<Class Id=\"Player\" Type=\"TYPE_PLAYER\" Path=\"NFDataCfg/Struct/Class/Player.xml\" InstancePath=\"\"/>"
        "</Class></XML>";
    pm.files["NFDataCfg/Struct/Class/IObject.xml"] =
        "<XML><Propertys>" + prop("ClassName", "string") + prop("ConfigID", "string") + "</Propertys></XML>";
    for (const char* c : {"NPC", "Player"})
        pm.files[std::string("NFDataCfg/Struct/Class/") + c + ".xml"] =
            "<XML><Propertys>" + prop("SceneID", "int") + prop("GroupID", "int") + prop("X", "float") + prop("Y", "float") +
            prop("Z", "float") + "</Propertys><Records></Records></XML>";

    TestLogModule log;
    NFCClassModule classes(&pm);
    NFCElementModule elements(&pm);
    ViewKernel kernel(&pm);
    NFCScheduleModule sched(&pm);
    NFCSceneAOIModule aoi(&pm);
    NFCEventModule events(&pm);
    pm.AddModule(typeid(NFILogModule).name(), &log);
    pm.AddModule(typeid(NFIClassModule).name(), &classes);
    pm.AddModule(typeid(NFIElementModule).name(), &elements);
    pm.AddModule(typeid(NFIKernelModule).name(), &kernel);
    pm.AddModule(typeid(NFISceneAOIModule).name(), &aoi);
    pm.AddModule(typeid(NFIEventModule).name(), &events);
    pm.AddModule(typeid(NFIScheduleModule).name(), &sched);
    std::vector<NFIModule*> all = {&log, &classes, &elements, &kernel, &aoi, &events, &sched};
    for (auto* m : all) m->Awake();
    for (auto* m : all) m->Init();  // (the AOI module's common callbacks stay registered)
    NFIKernelModule* km = &kernel;
    NFISceneAOIModule* am = &aoi;
    Printer printer;
    am->AddObjectEnterCallBack(&printer, &Printer::OnEnter);
    am->AddObjectLeaveCallBack(&printer, &Printer::OnLeave);

    std::map<int, int> groups;  // scene -> its highest group
    auto create = [&](int i, const std::string& cls, int s, int g) {
        g_index[guid_of(i)] = i;
        return (bool)km->CreateObject(guid_of(i), s, g, cls == "P" ? "Player" : "NPC", "", NFCDataList());
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
            if (!km->CreateScene(I(1))) return 3;
            groups[I(1)] = 0;
        } else if (op == "GRP") {
            while (groups[I(1)] < I(2))
                if (km->RequestGroupScene(I(1)) != ++groups[I(1)]) return 3;
        } else if (op == "OBJ" || op == "CR") {
            if (!create(I(1), f[2], I(3), I(4))) return 4;
        } else if (op == "INIT") {
            for (auto* m : all) m->AfterInit();
            for (auto* m : all) m->ReadyExecute();
            g_print = true;
        } else if (op == "SW") {
            if (!km->SwitchScene(guid_of(I(1)), I(2), I(3), 1.0f, 2.0f, 3.0f, 0.0f, NFCDataList())) return 5;
        } else if (op == "DE") {
            if (!km->DestroyObject(guid_of(I(1)))) return 6;
        } else if (op != "X") {
            return 7;
        }
    }
    return 0;
}
