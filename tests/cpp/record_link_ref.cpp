// record_link_ref.cpp — the reference's own answers on NFCPropertyModule::OnRecordPropertyEvent, for
// tests/golden/record_link.json.  NFCPropertyModule.cpp is compiled where it lies, with the reference's
// kernel, AOI, event, schedule, class and element modules, around oracle/ref_server.hpp's plugin manager;
// the two interfaces the module also asks for (NFIPropertyConfigModule, NFILevelModule) are doubles of
// this harness: the base values of a level are whatever the script's last BASE / LV line handed over.
// The Player class is written here: the int properties Level, Job, HP, MP, SP, OnlineCount, SceneID,
// GroupID and one per column tag (none for a tag that starts with '_': an unlinked column), and the
// record CommPropertyValue of ROWS x COLS int columns tagged with those names.  The script of tests/record_link_model.py (golden_script()):
//   SHAPE <rows> <cols>            TAGS <name> x cols          BASE <v> x cols         OBJ <n>
//   SV / AV / UV <o> <group> <name> <v>   the module's SetPropertyValue / AddPropertyValue / SubPropertyValue
//   SI <o> <row> <col> <v> | AR <o> <row> [v x cols] | RM <o> <row> | CL <o> | SW <o> <origin> <target>
//                                  FindRecord(...)->SetInt / AddRow / Remove / Clear / SwapRowInfo
//   LV <o> <level> <v x cols>      SetPropertyInt(self, "Level", level): the module's level callback
//                                  rewrites row NPG_JOBLEVEL of every column with the base values v
//   X                              the frame (the reference applies a call at once: nothing here)
// Objects are created through NFCKernelModule::CreateObject, so the module's own class callback adds the
// rows and sets Level 1 (base values: the BASE line).  Every call line prints
//   A <k> <ret> : <GetPropertyInt of every tag's property of object o, in column order>
// and, first, the line "I : <the same values right after creation>" once per object.
// TEST INFRASTRUCTURE, run by tests/golden/gen_record_link_golden.py on a machine that has the reference.
//
// usage: record_link_ref <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "NFComm/NFConfigPlugin/NFCClassModule.h"
#include "NFComm/NFConfigPlugin/NFCElementModule.h"
#include "NFComm/NFCore/NFCDataList.h"
#include "NFComm/NFKernelPlugin/NFCEventModule.h"
#include "NFComm/NFKernelPlugin/NFCKernelModule.h"
#include "NFComm/NFKernelPlugin/NFCScheduleModule.h"
#include "NFComm/NFKernelPlugin/NFCSceneAOIModule.h"
#include "NFServer/NFGameServerPlugin/NFCPropertyModule.h"
#include "ref_server.hpp"

static std::vector<std::string> g_tags;
static std::vector<long long> g_base;  // the base value of each tag at the next level callback

class BaseValues : public NFIPropertyConfigModule {
public:
    int CalculateBaseValue(const int, const int, const std::string& tag) override {
        for (size_t c = 0; c < g_tags.size(); c++)
            if (g_tags[c] == tag) return (int)g_base[c];
        return 0;
    }
    bool LegalLevel(const int, const int) override { return true; }
};
class NoLevels : public NFILevelModule {
public:
    int AddExp(const NFGUID&, const int) override { return 0; }
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<std::vector<std::string>> lines;
    for (std::string ln; std::getline(in, ln);) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (!f.empty()) lines.push_back(f);
    }
    int rows = 0, cols = 0, n_obj = 0;
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "SHAPE") {
            rows = atoi(f[1].c_str());
            cols = atoi(f[2].c_str());
        } else if (f[0] == "TAGS") {
            g_tags.assign(f.begin() + 1, f.end());
        } else if (f[0] == "BASE") {
            for (size_t c = 1; c < f.size(); c++) g_base.push_back(strtoll(f[c].c_str(), nullptr, 10));
        } else if (f[0] == "OBJ") {
            n_obj = atoi(f[1].c_str());
        } else {
            break;
        }
    }
    if (rows <= 0 || (int)g_tags.size() != cols || (int)g_base.size() != cols || n_obj <= 0) return 2;

    TestPluginManager pm;
    auto prop = [](const std::string& id, const char* type) {
        return "<Property Id=\"" + id + "\" Type=\"" + type + "\" Public=\"0\" Private=\"1\" Save=\"0\" Cache=\"0\" Ref=\"0\" Upload=\"0\"/>";
    };
    pm.files["NFDataCfg/Struct/LogicClass.xml"] =
        "<XML><Class Id=\"IObject\" Type=\"TYPE_IOBJECT\" Path=\"NFDataCfg/Struct/Class/IObject.xml\" InstancePath=\"\">"
        "<Class Id=\"Player\" Type=\"TYPE_PLAYER\" Path=\"NFDataCfg/Struct/Class/Player.xml\" InstancePath=\"\"/></Class></XML>";
    pm.files["NFDataCfg/Struct/Class/IObject.xml"] =
        "<XML><Propertys>" + prop("ClassName", "string") + prop("ConfigID", "string") + "</Propertys></XML>";
    {
        std::string x = "<XML><Propertys>";
        for (const char* nm : {"Level", "Job", "HP", "MP", "SP", "OnlineCount", "SceneID", "GroupID"}) x += prop(nm, "int");
        for (auto& t : g_tags)
            if (t[0] != '_') x += prop(t, "int");  // (a tag that starts with '_' names no property: an unlinked column)
        x += "</Propertys><Records><Record Id=\"CommPropertyValue\" Row=\"" + std::to_string(rows) + "\" Col=\"" +
             std::to_string(cols) + "\" Public=\"0\" Private=\"1\" Save=\"0\" Cache=\"0\" Upload=\"0\">";
        for (auto& t : g_tags) x += "<Col Type=\"int\" Tag=\"" + t + "\"/>";
        x += "</Record></Records></XML>";
        pm.files["NFDataCfg/Struct/Class/Player.xml"] = x;
    }
    TestLogModule log;
    NFCClassModule classes(&pm);
    NFCElementModule elements(&pm);
    NFCKernelModule kernel(&pm);
    NFCSceneAOIModule aoi(&pm);
    NFCEventModule events(&pm);
    NFCScheduleModule sched(&pm);
    BaseValues base;
    NoLevels levels;
    NFCPropertyModule props(&pm);
    pm.AddModule(typeid(NFILogModule).name(), &log);
    pm.AddModule(typeid(NFIClassModule).name(), &classes);
    pm.AddModule(typeid(NFIElementModule).name(), &elements);
    pm.AddModule(typeid(NFIKernelModule).name(), &kernel);
    pm.AddModule(typeid(NFISceneAOIModule).name(), &aoi);
    pm.AddModule(typeid(NFIEventModule).name(), &events);
    pm.AddModule(typeid(NFIScheduleModule).name(), &sched);
    pm.AddModule(typeid(NFIPropertyConfigModule).name(), &base);
    pm.AddModule(typeid(NFILevelModule).name(), &levels);
    pm.AddModule(typeid(NFIPropertyModule).name(), &props);
    std::vector<NFIModule*> all = {&log, &classes, &elements, &kernel, &aoi, &events, &sched, &base, &levels, &props};
    for (auto* m : all) m->Awake();
    for (auto* m : all) m->Init();
    for (auto* m : all) m->AfterInit();
    NFIKernelModule* km = &kernel;
    NFIPropertyModule* pmod = &props;
    km->CreateScene(1);
    if (km->RequestGroupScene(1) != 1) return 3;
    auto guid = [](int o) { return NFGUID(7, 100 + o); };
    const std::string rec = "CommPropertyValue";
    auto print_props = [&](int o) {
        for (auto& t : g_tags) printf(" %lld", (long long)km->GetPropertyInt(guid(o), t));
        printf("\n");
    };
    for (int o = 0; o < n_obj; o++) {
        if (!km->CreateObject(guid(o), 1, 1, "Player", "", NFCDataList())) return 3;
        printf("I :");
        print_props(o);
    }
    int k = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") continue;
        const int o = atoi(f[1].c_str());
        const NFGUID g = guid(o);
        NF_SHARE_PTR<NFIRecord> R = km->FindRecord(g, rec);
        if (!R) return 3;
        long long ret = 0;
        if (op == "SV" || op == "AV" || op == "UV") {
            const NFIPropertyModule::NFPropertyGroup grp = (NFIPropertyModule::NFPropertyGroup)atoi(f[2].c_str());
            const int v = (int)strtoll(f[4].c_str(), nullptr, 10);
            ret = op == "SV" ? pmod->SetPropertyValue(g, f[3], grp, v)
                : op == "AV" ? pmod->AddPropertyValue(g, f[3], grp, v) : pmod->SubPropertyValue(g, f[3], grp, v);
        } else if (op == "SI") {
            ret = R->SetInt(atoi(f[2].c_str()), atoi(f[3].c_str()), (NFINT64)strtoll(f[4].c_str(), nullptr, 10));
        } else if (op == "AR") {
            if (f.size() > 3) {
                NFCDataList v;
                for (size_t c = 3; c < f.size(); c++) v.Add((NFINT64)strtoll(f[c].c_str(), nullptr, 10));
                ret = R->AddRow(atoi(f[2].c_str()), v);
            } else {
                ret = R->AddRow(atoi(f[2].c_str()));
            }
        } else if (op == "RM") {
            ret = R->Remove(atoi(f[2].c_str()));
        } else if (op == "CL") {
            ret = R->Clear();
        } else if (op == "SW") {
            ret = R->SwapRowInfo(atoi(f[2].c_str()), atoi(f[3].c_str()));
        } else if (op == "LV") {
            for (int c = 0; c < cols; c++) g_base[c] = strtoll(f[3 + c].c_str(), nullptr, 10);
            ret = km->SetPropertyInt(g, "Level", (NFINT64)strtoll(f[2].c_str(), nullptr, 10));
        } else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
        printf("A %d %lld :", k++, ret);
        print_props(o);
    }
    return 0;
}
